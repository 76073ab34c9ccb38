"""The round of csrc/ordered_scan.h: ordered_scan walks SCAN_ROUND counts between two barriers.  The GPU tests build their boundary
cases from this constant (an array of SCAN_ROUND - 1, SCAN_ROUND and SCAN_ROUND + 1 counts: the last full round, and the first count
of a second one); tests/test_scan_round.py holds it against the header's text, so that a change of kScanRound cannot leave those
cases off the boundary unnoticed."""
import re

from tests import abi_text

SCAN_ROUND = 4096
BLOCK = 256            # items per workgroup of the passes whose counts are scanned (csrc/common.h: kBlock)


def header_scan_round() -> int:
    """kScanRound as csrc/ordered_scan.h states it"""
    found = re.findall(r"^constexpr int kScanRound = (\d+);", abi_text.source("ordered_scan.h"), re.M)
    assert len(found) == 1, found
    return int(found[0])
