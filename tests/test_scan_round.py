"""The constant the GPU boundary cases of the ordered scan are built from is the one the kernels are compiled with.  CPU only."""
import re

from tests import abi_text, scan_round


def test_the_boundary_cases_are_built_from_the_header_s_round():
    assert scan_round.header_scan_round() == scan_round.SCAN_ROUND
    text = abi_text.source("ordered_scan.h")
    block = int(re.search(r"^constexpr int kScanBlock = (\d+);", text, re.M).group(1))
    assert scan_round.SCAN_ROUND % block == 0                       # a whole number of counts per thread
    assert int(re.search(r"^constexpr int kBlock = (\d+);", abi_text.source("common.h"), re.M).group(1)) == scan_round.BLOCK


def test_every_boundary_case_reaches_a_second_round():
    """the shapes the GPU tests derive from SCAN_ROUND, restated: the length of the array each scan walks"""
    from tests import densify_reference, moran_reference, triplane_reference
    R = scan_round.SCAN_ROUND
    assert {n for kind, n, _ in moran_reference.KNN_CLOUDS if kind == "uniform"} >= {R - 1, R, R + 1}
    blocks = lambda n: (n + scan_round.BLOCK - 1) // scan_round.BLOCK
    rows = lambda case: case["params"]["xyz"].shape[0]
    assert 4 * blocks(rows(densify_reference.full_scan_pass_case())) == R            # four counts per workgroup: R + 4 is the next length
    assert 4 * blocks(rows(densify_reference.second_scan_pass_case())) == R + 4
    c = triplane_reference.CASE_BY_NAME[triplane_reference.SCAN_CASE]
    tiles = ((c.H + 15) // 16) * ((c.W + 15) // 16)                                   # C <= 32: tiles of 16 x 16 texels
    assert c.C <= 32 and 96 * (tiles - 1) <= R < 96 * tiles                          # 3 planes x 32 copies per tile: the first tile count beyond R
