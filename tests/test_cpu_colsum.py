"""CPU: the row partition and workspace sizes behind the fixed-order column sums (cdsegnet_amd/csrc/colsum.h) as the library
exports them - cdseg_bn_partition / cdseg_bn_ws_bytes (csrc/norm.hip), cdseg_fuse_gate_ws_bytes (csrc/fusion.hip),
cdseg_skip_partition / cdseg_skip_stats_ws_bytes (csrc/skip.hip) - against the one restated rule of tests/colsum_rule.py, in
both builds; unsupported input gives the status and leaves the outputs alone, or gives 0 bytes.  Host code, no launch."""
import ctypes

import pytest

from cdsegnet_amd import _lib
from tests import colsum_rule as R

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
MS = [0, 1, 63, 64, 65, 255, 256, 257, 16384, 16385, 65536, 65537, 5003, 20000, 33001, 120000, 2600000]
BN_OK, BN_BAD = [16, 32, 48, 64, 128, 256, 496, 512], [-16, 0, 1, 8, 24, 36, 511, 528, 1024]
ANY_OK, ANY_BAD = [1, 3, 30, 32, 36, 48, 128, 511, 512], [-1, 0, 513, 516, 1024]


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


def _partition(fn, m, c):
    rows, blocks = ctypes.c_long(-7), ctypes.c_int(-7)
    return fn(m, c, ctypes.byref(rows), ctypes.byref(blocks)), rows.value, blocks.value


def test_exported_partitions_and_workspaces_follow_the_one_rule(lib):
    ops = ((lib.cdseg_bn_partition, lib.cdseg_bn_ws_bytes, 2, R.MIN_ROWS_BN, BN_OK, BN_BAD),
           (None, lib.cdseg_fuse_gate_ws_bytes, 2, R.MIN_ROWS_SWEEP, ANY_OK, ANY_BAD),
           (lib.cdseg_skip_partition, lib.cdseg_skip_stats_ws_bytes, 3, R.MIN_ROWS_SWEEP, ANY_OK, ANY_BAD))
    for part, ws_bytes, nsums, min_rows, good, bad in ops:
        for m in MS:
            rpb, blocks = R.partition(m, min_rows)
            assert blocks <= 256 and (rpb == min_rows or rpb % 64 == 0) and (m == 0 or (blocks - 1) * rpb < m <= blocks * rpb)
            for c in good:
                assert part is None or _partition(part, m, c) == (OK, rpb, blocks), (m, c)
                assert ws_bytes(m, c) == R.ws_bytes(m, nsums, c, min_rows) == blocks * nsums * c * 8, (m, c)
            for c in bad:
                assert part is None or _partition(part, m, c) == (ERR_UNSUPPORTED, -7, -7), (m, c)
                assert ws_bytes(m, c) == 0, (m, c)
        for c in good + bad:  # a negative row count: an argument error before the width is looked at, and no bytes
            assert part is None or _partition(part, -1, c) == (ERR_ARG, -7, -7), c
            assert ws_bytes(-1, c) == 0, c
        if part is not None:
            assert part(100, good[0], None, None) == ERR_ARG
            rows = ctypes.c_long(-7)
            assert part(100, good[0], ctypes.byref(rows), None) == ERR_ARG and rows.value == -7


def test_ops_return_one_named_partition_type():
    from cdsegnet_amd import ops
    bn, sk = ops.bn_partition(5003, 32), ops.skip_partition(2100, 32)
    assert type(bn) is type(sk) and isinstance(sk, tuple)
    assert (bn.rows_per_block, bn.blocks) == tuple(bn) == (256, 20)
    assert (sk.rows_per_block, sk.blocks) == tuple(sk) == (sk[0], sk[1]) == (64, 33)
