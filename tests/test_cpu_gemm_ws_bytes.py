"""CPU: the one rule that sizes cdseg_gemm's workspace (csrc/workspace.h) through its three consumers - the public query
cdseg_gemm_ws_bytes, the native Block executor's scratch (csrc/runtime.hip) and the training Block's scratch
(csrc/trainblock.hip).  The size functions are host code: they load and answer without a device.  Every figure below is a
literal: the query's at the edges of the rule's gates, the two Blocks' as recorded from the commit before the rule moved (where
ops.gemm, runtime.hip and trainblock.hip each carried a copy of it), so a change of the rule shows as a changed number."""
import ctypes

import pytest

from cdsegnet_amd import _lib

MIB = 1 << 20


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


@pytest.mark.parametrize("M,N,gathered,fused_ln,want", [
    (1, 16, 0, 0, 2048),                  # 32 planes of one row
    (800, 512, 0, 0, 52428800),           # 13 x 4 tiles of 64 x 128: 32 M N 4, below the cap
    (16320, 128, 0, 0, 64 * MIB),         # 255 tiles: the last M that splits (capped)
    (16321, 128, 0, 0, 0),                # 256 tiles: the grid fills the chip
    (8192, 256, 1, 0, 64 * MIB),          # 256 tiles of 64 x 128, 64 of 128 x 256: the deep-conv branch, 8 M N 4
    (8192, 256, 0, 0, 0),                 # the same shape, not gathered
    (32641, 256, 1, 0, 0),                # 256 tiles of 128 x 256
    (16384, 256, 0, 1, 16 * MIB),         # fused LayerNorm over two column tiles: one plane M N 4
    (16384, 128, 0, 1, 0),                # rows inside one column tile
])
def test_cdseg_gemm_ws_bytes_at_the_gate_edges(lib, M, N, gathered, fused_ln, want):
    assert lib.cdseg_gemm_ws_bytes(M, N, gathered, fused_ln) == want


def test_cdseg_gemm_ws_bytes_more_edges(lib):
    q = lib.cdseg_gemm_ws_bytes
    assert q(0, 128, 0, 0) == 0 and q(100, 0, 1, 1) == 0                      # an empty problem
    assert q(32640, 256, 1, 0) == 64 * MIB and q(8192, 255, 1, 0) == 0        # 255 deep tiles; N below a deep tile
    assert q(8192, 256, 1, 1) == 64 * MIB                                     # the split-K branches come first
    assert q(8193, 256, 0, 1) == 8193 * 256 * 4 and q(8193, 129, 0, 1) == 8193 * 129 * 4
    assert q(300000, 512, 0, 1) == 300000 * 512 * 4 > 64 * MIB                # the LayerNorm plane is needed whole: no cap
    assert q(100, 128, 0, 1) == q(100, 128, 0, 0) == 32 * 100 * 128 * 4


def _block_scratch(lib, C, n, dtype, imgs):
    d = _lib.BlockDesc()
    d.dtype, d.channels, d.heads, d.hidden = dtype, C, C // 16, 4 * C
    if imgs:
        d.head_img = d.tail_img = 4096  # (only their presence is read)
    return lib.cdseg_block_scratch_bytes(ctypes.byref(d), n)


@pytest.mark.parametrize("C,n,dtype,imgs,want", [
    (32, 900, _lib.BF16, 1, 15321600),       # few tiles: 32 planes of the widest product (fc1)
    (128, 2300, _lib.BF16, 1, 74174464),     # the same, capped at 64 MiB
    (128, 16321, _lib.BF16, 1, 50138112),    # 256 tiles, rows inside one column tile: no GEMM workspace
    (256, 8129, _lib.BF16, 1, 116537344),    # past the 64 x 128 gate: the conv's 8 planes
    (256, 8192, _lib.F32, 0, 150994944),
    (256, 32641, _lib.BF16, 1, 233970688),   # past both gates: the LayerNorm plane
    (512, 4033, _lib.BF16, 1, 115634176),
    (512, 3200, _lib.F32, 0, 132644864),
    (512, 120000, _lib.BF16, 1, 1541668864),
])
def test_cdseg_block_scratch_bytes_is_what_it_was(lib, C, n, dtype, imgs, want):
    assert _block_scratch(lib, C, n, dtype, imgs) == want


@pytest.mark.parametrize("C,n,mm,attn,det,want", [
    (32, 777, 0, 0, 0, [1791232, 13744896, 163840, 167424]),
    (128, 16321, 1, 1, 0, [108632576, 85136384, 2621440, 2630144]),
    (256, 8192, 1, 1, 1, [109051904, 172231680, 10485760, 10503168]),
    (256, 32641, 0, 0, 0, [601638912, 340523008, 10485760, 10503168]),
    (512, 4033, 1, 1, 0, [107374592, 150245376, 41943040, 41977856]),
    (512, 120000, 0, 1, 1, [4055040000, 2514227200, 41943040, 41977856]),
])
def test_cdseg_train_block_bytes_is_what_it_was(lib, C, n, mm, attn, det, want):
    t = _lib.TrainBlockDesc()
    t.channels, t.heads, t.hidden = C, C // 16, 4 * C
    t.mm_dtype, t.attn_dtype, t.deterministic = mm, attn, det
    out = [ctypes.c_size_t(0) for _ in range(4)]
    assert lib.cdseg_train_block_bytes(ctypes.byref(t), n, (n + 63) // 64 * 64, *[ctypes.byref(o) for o in out]) == 0
    assert [int(o.value) for o in out] == want  # tape, scratch, derived, gradient slab
