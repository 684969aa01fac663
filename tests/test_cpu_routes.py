"""CPU: the launch record of the C ABI (include/cdseg.h cdseg_route_*, csrc/route.h) - host code only, so its semantics are
checked without a GPU, in both builds of the library: the catalogue, enable / clear / read, the ring, and that the record is
per host thread.  Records are appended with cdseg_route_note, which goes through the same function as the recording sites in
front of the launches (tests/test_gpu_routes.py checks what those sites record)."""
import ctypes
import os
import threading

import pytest

from cdsegnet_amd import _lib, ops

RING = 64  # include/cdseg.h: "a ring of the newest 64 launches"

_TILES16 = ("1,1>", "1,2>", "1,4>", "2,1>", "2,2>", "2,4>", "4,1>", "4,2>")  # csrc/wgrad_partition.h partition_16
_WIDTHS = ("16,1>", "16,2>", "64,1>", "64,2>", "64,4>")                      # csrc/loss.hip launch_by_width
_LP = ("b16>", "f32>")
OTHER_FAMILIES = {
    "layernorm_kernel<": ("1>", "2>", "4>", "8>"),
    "add_layernorm_kernel<": tuple(f"{mv},{t}" for mv in (1, 2, 4, 8) for t in _LP),
    "gather_first_kernel<": _LP, "scatter_first_kernel<": ("acc>", "set>"), "scale_cast_kernel<": _LP,
    "gelu_fwd_kernel<": _LP, "gelu_bwd_cast_kernel<": _LP,
    "wgrad_kernel": ("",), "wgrad_det_kernel": ("",), "wgrad16_kernel<": _TILES16, "wgrad16_det_kernel<": _TILES16,
    "attn_bwd_q_mfma_kernel<": (">", "DropP>"), "attn_bwd_kv_mfma_kernel<": (">", "DropP>"),
    "attn_bwd16_q_kernel<": (">", "DropP>"), "attn_bwd16_kv_kernel<": (">", "DropP>"),
    "layernorm_bwd_kernel": ("",), "layernorm_bwd_det_kernel": ("",),
    "pool_fused_kernel<": ("32,64,walk>", "32,64,scan>", "64,128,walk>", "64,128,scan>"),
    "unpool_fused_kernel<": ("32,64>", "64,128>"),
    "loss_rows_kernel<": _WIDTHS, "loss_bwd_kernel<": _WIDTHS,
    "sk_stats_kernel<": _LP, "sk_stats_scalar_kernel<": _LP, "sk_fold_kernel<": _LP, "sk_merge_kernel": ("",),
    "sk_merge_scalar_kernel": ("",),
    "fg_fwd_kernel": ("",), "fg_fwd_scalar_kernel": ("",), "fg_bwd_kernel": ("",), "fg_bwd_scalar_kernel": ("",),
}


@pytest.fixture(scope="module", params=_lib.VARIANTS)
def lib(request):
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.LIB_PATH_F16)):
        from cdsegnet_amd.build import build_library
        build_library()
    return _lib.load(request.param)


@pytest.fixture(autouse=True)
def _recording_off_afterwards(lib):
    yield
    lib.cdseg_route_enable(0)
    lib.cdseg_route_clear()


def _note(lib, *words):
    rec = (ctypes.c_int32 * 8)(*words)
    return lib.cdseg_route_note(rec)


def _read(lib, capacity):
    rec = (ctypes.c_int32 * (8 * max(capacity, 1)))(*([-7] * (8 * max(capacity, 1))))
    count = lib.cdseg_route_read(rec, capacity)
    return count, [list(rec[8 * i:8 * i + 8]) for i in range(max(capacity, 1))]


def test_catalogue_names_are_unique_and_the_same_in_both_builds(lib):
    names = ops.route_catalog(lib)
    assert len(names) > 40 and all(names), names
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert all(n == n.strip() and "\n" not in n for n in names)
    assert names == ops.route_catalog(_lib.load("bf16"))  # same sources: an id means the same kernel in either build
    # every chooser the record covers has at least one kernel in it
    for family in ("gemm_kernel<", "gemm_dma_kernel<", "mlp_fused_kernel<", "cpe_head_fused_kernel<", "cpe_head_stream_kernel<",
                   "deep_head_kernel<", "deep_tail_kernel<", "head_rr_kernel<", "tail_rr_kernel<", "conv_ll_kernel<", "attn_"):
        assert any(n.startswith(family) for n in names), family
    # the choosers outside the GEMM and the Block: family -> the instantiations its launcher can pick, every one of them
    for family, arms in OTHER_FAMILIES.items():
        assert sorted(n for n in names if n.startswith(family)) == sorted(family + a for a in arms), family
    # a buffer that is too small is left alone; the size asked for is the size needed
    need = lib.cdseg_route_catalog(None, 0)
    assert need == len("\n".join(names)) + 1
    buf = ctypes.create_string_buffer(b"\x55" * need, need)
    assert lib.cdseg_route_catalog(buf, need - 1) == need and buf.raw == b"\x55" * need
    assert lib.cdseg_route_catalog(buf, need) == need and buf.raw[-1:] == b"\0" and buf.value.decode() == "\n".join(names)


def test_enable_clear_read(lib):
    assert lib.cdseg_route_enable(0) == 0  # off by default (the fixture leaves it off)
    lib.cdseg_route_clear()
    assert _note(lib, 3, 64, 32, 1, 0, 0, 1, 0) == 0
    assert _read(lib, 4)[0] == 0, "recording is off: a site records nothing"
    assert lib.cdseg_route_enable(1) == 0
    assert lib.cdseg_route_enable(5) == 1  # returns the previous state; any non-zero value is "on"
    assert _note(lib, 3, 64, 32, 1, 0, 0, 1, 0) == 0
    assert _note(lib, 5, 128, 128, 4, 1, 2, 0x23, 9) == 0
    count, rows = _read(lib, 4)
    assert count == 2
    assert rows[0] == [3, 64, 32, 1, 0, 0, 1, 0] and rows[1] == [5, 128, 128, 4, 1, 2, 0x23, 9]
    assert rows[2] == [-7] * 8 and rows[3] == [-7] * 8, "nothing is written past the records there are"
    assert _read(lib, 4)[0] == 2, "reading does not consume"
    # capacity below the count: the newest ones, oldest first
    count, rows = _read(lib, 1)
    assert count == 2 and rows[0] == [5, 128, 128, 4, 1, 2, 0x23, 9]
    # capacity 0 (and a NULL buffer): only the count
    count, rows = _read(lib, 0)
    assert count == 2 and rows[0] == [-7] * 8
    assert lib.cdseg_route_read(None, 0) == 2 and lib.cdseg_route_read(None, 8) == 2
    # switching off keeps what was recorded; clear forgets it and leaves the switch alone
    assert lib.cdseg_route_enable(0) == 1
    assert _read(lib, 4)[0] == 2
    lib.cdseg_route_enable(1)
    lib.cdseg_route_clear()
    assert _read(lib, 4)[0] == 0
    assert lib.cdseg_route_enable(1) == 1
    # an id outside the catalogue is refused and records nothing
    n = len(ops.route_catalog(lib))
    assert _note(lib, n, 0, 0, 0, 0, 0, 0, 0) == -1 and _note(lib, -1, 0, 0, 0, 0, 0, 0, 0) == -1
    assert lib.cdseg_route_note(None) == -1
    assert _read(lib, 4)[0] == 0


@pytest.mark.parametrize("total", [RING - 1, RING, RING + 1, 2 * RING + 5])
def test_ring_keeps_the_newest_records_in_order(lib, total):
    assert RING >= 32  # one cdseg_block_forward fits
    lib.cdseg_route_enable(1)
    lib.cdseg_route_clear()
    for i in range(total):
        assert _note(lib, i % 7, i, 2 * i, 3, 1, 2, i & 63, -i) == 0
    kept = min(total, RING)
    count, rows = _read(lib, RING + 8)
    assert count == total, "the count goes on past the ring"
    want = [[i % 7, i, 2 * i, 3, 1, 2, i & 63, -i] for i in range(total - kept, total)]
    assert rows[:kept] == want
    assert rows[kept:] == [[-7] * 8] * (RING + 8 - kept)
    for cap in (1, 5, RING - 1):
        count, rows = _read(lib, cap)
        assert count == total and rows[:cap] == want[kept - min(cap, kept):][:cap]
    # the python wrapper resolves ids to names
    count, routes = ops.route_read(lib)
    names = ops.route_catalog(lib)
    assert count == total and [r.kernel for r in routes] == [names[w[0]] for w in want]
    assert routes[-1].bm == total - 1 and routes[-1].aux == -(total - 1)


def test_record_is_per_host_thread(lib):
    lib.cdseg_route_enable(1)
    lib.cdseg_route_clear()
    _note(lib, 1, 1, 1, 1, 0, 0, 0, 0)
    seen = {}

    def other():
        seen["was_on"] = lib.cdseg_route_enable(1)  # a new thread starts with recording off and an empty ring
        seen["count0"] = lib.cdseg_route_read(None, 0)
        _note(lib, 2, 2, 2, 1, 0, 0, 0, 0)
        _note(lib, 2, 2, 2, 1, 0, 0, 0, 0)
        seen["count"] = lib.cdseg_route_read(None, 0)

    t = threading.Thread(target=other)
    t.start(); t.join()
    assert seen == {"was_on": 0, "count0": 0, "count": 2}
    count, rows = _read(lib, 4)
    assert count == 1 and rows[0][0] == 1


def test_route_flag_bits_of_the_python_wrapper_match_the_header():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cdseg.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define CDSEG_ROUTE_(\w+) (\d+)", hdr)}
    assert vals == {"WORDS": ops.ROUTE_WORDS, "F_VEC_OK": ops.ROUTE_F_VEC_OK, "F_GATHER": ops.ROUTE_F_GATHER,
                    "F_PARTIALS": ops.ROUTE_F_PARTIALS, "F_KDIV": ops.ROUTE_F_KDIV, "F_KSHIFT_LT6": ops.ROUTE_F_KSHIFT_LT6,
                    "F_CT_SHIFT": ops.ROUTE_F_CT_SHIFT}
    r = ops.Route("k", 64, 32, 2, 1, 0, 1 | 2 | 8 | (2 << 5), 0)
    assert r.vec_ok and r.gather and r.kdiv and not r.partials and not r.kshift_lt6 and r.compute == 2
