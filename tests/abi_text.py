"""What the ABI tests read as text: include/splatraster.h parsed once (prototypes, structs, #define values), and the definition of
an entry point, found in whichever file of build.SOURCES holds it."""
import functools
import os
import re

from splatfields_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "splatfields_amd", "csrc")


@functools.lru_cache(maxsize=None)
def header():
    """include/splatraster.h without comments (build.strip_comments: one declaration may still span several lines)"""
    return build.strip_comments(open(os.path.join(ROOT, "include", "splatraster.h")).read())


@functools.lru_cache(maxsize=None)
def source(name):
    """the text of one file under csrc/, comments included"""
    return open(os.path.join(CSRC, name)).read()


def _declarators(rest):
    """`*a, *b`, `height, width`, `m[12]` -> [(pointer stars, name, array length or None), ...]"""
    out = []
    for d in rest.split(","):
        m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d)
        assert m, rest
        out.append((m.group(1), m.group(2), int(m.group(3)) if m.group(3) else None))
    return out


@functools.lru_cache(maxsize=None)
def structs():
    """{struct name: [(type text, field name, array length or None), ...]} in declaration order; `const float *a, *b;` gives
    two fields of type `const float*`"""
    out = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} (\w+);", header(), re.S):
        assert m.group(1) == m.group(3), m.group(1)
        fields = []
        for decl in (d.strip() for d in m.group(2).split(";")):
            if not decl:
                continue
            base, rest = re.fullmatch(r"((?:const )?(?:unsigned(?: (?:int|char|long long))?|long long|\w+))\s*(.*)", decl, re.S).groups()
            for stars, name, length in _declarators(rest):
                fields.append((base + stars, name, length))
        out[m.group(1)] = fields
    return out


@functools.lru_cache(maxsize=None)
def defines():
    """{name: value text} of every object-like #define that has a value (the include guard has none)"""
    return {m.group(1): m.group(2).strip() for m in re.finditer(r"^#define (\w+) (.+)$", header(), re.M)}


@functools.lru_cache(maxsize=None)
def prototypes():
    """{function name: (return type, [argument declaration, ...])}; `(void)` is an empty list"""
    text = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", header(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.startswith("#") and line not in ('extern "C" {', "}"))
    out = {}
    for stmt in (s.strip() for s in text.split(";")):
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, re.S)
        assert m, stmt
        args = [" ".join(a.split()) for a in m.group(3).split(",")]
        assert m.group(2) not in out, m.group(2)
        out[m.group(2)] = (m.group(1).strip(), [] if args == ["void"] else args)
    return out


def entry_point(name):
    """the text of the one definition of `name` among build.SOURCES: from its return type in column 0 to the closing brace in
    column 0, or a one-line definition"""
    pattern = r"^[a-z_][a-z_ ]*\*? %s\([^;{]*\{(?:[^\n]*\}$|.*?^\}$)" % re.escape(name)
    found = [m.group(0) for f in build.SOURCES for m in re.finditer(pattern, source(f), re.S | re.M)]
    assert len(found) == 1, (name, len(found))
    return found[0]

