"""splatfields_amd/build.py lists the headers the library is built from by hand (HEADERS feeds the staleness check and
source_hash): every file a source reaches through #include "..." must be on that list."""
import os
import re

from splatfields_amd import build


def reachable_includes():
    found, todo = set(), [os.path.join(str(build.CSRC), f) for f in build.SOURCES]
    while todo:
        path = todo.pop()
        for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', build.strip_comments(open(path).read()), re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(path), name))
            if target not in found:
                found.add(target)
                todo.append(target)
    return found


def test_every_included_header_is_listed():
    listed = {os.path.normpath(os.path.join(str(build.CSRC), h)) for h in build.HEADERS}
    reached = reachable_includes()
    assert os.path.join(str(build.CSRC), "common.h") in reached            # the walk finds something
    assert reached <= listed, sorted(os.path.relpath(p, str(build.CSRC)) for p in reached - listed)
    for path in listed:
        assert os.path.isfile(path), path
