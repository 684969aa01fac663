"""CPU: the boundary of the native training Block (`DefaultSegmentorV2.train_block = "native"`, csrc/trainblock.hip) - what can
be checked without a device: the mode switch, the ABI, the argument checks (they run before any launch), the host-only size
query, and the autograd wiring of `train_graph._NativeBlock` on the emulated op layer (tests/emu_block_ops.py)."""
import ctypes
import os
import re

import pytest
import torch

from cdsegnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cdseg_train_block_bytes", "cdseg_train_block_grad_offsets", "cdseg_train_block_prepare", "cdseg_train_block_forward",
       "cdseg_train_block_backward", "cdseg_residual", "cdseg_scale_cast", "cdseg_add_layernorm", "cdseg_gelu_fwd",
       "cdseg_gelu_bwd_cast")


@pytest.fixture(params=list(_lib.VARIANTS))
def lib(request):
    return _lib.load(request.param)


# ------------------------------------------------------------------------------------------ mode
def test_train_block_mode_validation():
    import cdsegnet_amd.models  # noqa: F401
    from cdsegnet_amd import configs
    from cdsegnet_amd.registry import build_model
    from cdsegnet_amd.train_graph import TRAIN_BLOCKS, resolve_train_block
    assert TRAIN_BLOCKS == ("autograd", "native")
    model = build_model(configs.mini_config())
    assert model.train_block == "autograd" and resolve_train_block(model) == "autograd"
    assert "train_block" not in model.state_dict()
    model.train_block = "native"
    assert resolve_train_block(model) == "native"
    for bad in ("fused", "Native", None, True, 1):
        model.train_block = bad
        with pytest.raises(ValueError, match="train_block"):
            resolve_train_block(model)
    model.train()
    with pytest.raises(ValueError, match="train_block"):  # read at every forward, before anything else is touched
        model(dict(feat=torch.zeros(4, 6), coord=torch.zeros(4, 3), grid_coord=torch.zeros(4, 3, dtype=torch.int64),
                   offset=torch.tensor([4]), segment=torch.zeros(4, dtype=torch.int64)))


# ------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_binding_binds_the_new_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "cdseg.h")).read()
    declared = set(re.findall(r"\b(cdseg_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.cdseg_abi_version() == 1  # additive
    # the ctypes mirrors follow the header's field order
    for struct, cname in ((_lib.TrainBlockDesc, "cdseg_train_block_desc"), (_lib.TrainBlockIO, "cdseg_train_block_io")):
        body = hdr[hdr.index("typedef struct %s {" % cname):hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        order = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?\s*[;,]", body)
        assert order == [f[0] for f in struct._fields_], (order, cname)
    assert ctypes.sizeof(_lib.TrainBlockDesc) == 3 * 4 + 4 * 4 + 3 * 4 + 18 * 8 + 6 * 8 + 16


# ------------------------------------------------------------------------------------------ argument checks
BUF, ODD = 1 << 20, (1 << 20) + 8


def _desc(c=32, heads=2, hidden=128, mm=0, attn=0, det=0):
    d = _lib.TrainBlockDesc()
    d.channels, d.heads, d.hidden = c, heads, hidden
    d.attn_scale, d.eps_cpe, d.eps_norm1, d.eps_norm2 = 0.25, 1e-5, 1e-5, 1e-5
    d.mm_dtype, d.attn_dtype, d.deterministic = mm, attn, det
    for i in range(18):
        d.param[i] = BUF
    d.derived, d.derived_bytes = BUF, 1 << 40
    return d


def _io(n=100, slots=128):
    io = _lib.TrainBlockIO()
    io.n = n
    io.x_in = io.x_conv = io.x_out = io.tape = io.scratch = BUF
    io.nbr = io.gidx = io.widx = io.patch_start = BUF
    io.num_patches, io.max_len, io.num_slots = 2, 64, slots
    io.tape_bytes = io.scratch_bytes = 1 << 40
    return io


def _sizes(lib, d, n, slots):
    out = [ctypes.c_size_t(0) for _ in range(4)]
    assert lib.cdseg_train_block_bytes(ctypes.byref(d), n, slots, *[ctypes.byref(o) for o in out]) == 0
    return [int(o.value) for o in out]


def test_entry_points_check_their_arguments_before_any_launch(lib):
    """Pointers are never dereferenced on these paths: aligned non-null integers stand in for device memory.  Every case
    below must come back as CDSEG_ERR_ARG (a case that passed the checks would launch on a machine without a device)."""
    fwd, bwd, prep = lib.cdseg_train_block_forward, lib.cdseg_train_block_backward, lib.cdseg_train_block_prepare
    ref = ctypes.byref

    def both(d, io):
        return (fwd(ref(d), ref(io), None), bwd(ref(d), ref(io), BUF, BUF, BUF, None, BUF, None))

    d, io = _desc(), _io()
    io0 = _io(n=0)
    assert both(d, io0) == (0, 0)                                                  # n = 0: nothing to do
    assert fwd(None, ref(io), None) == -1 and fwd(ref(d), None, None) == -1 and bwd(None, ref(io), BUF, BUF, BUF, None, BUF, None) == -1
    assert prep(None, None) == -1
    for kw in (dict(c=40, heads=2), dict(c=24, heads=2), dict(hidden=100), dict(c=32, heads=1), dict(c=64, heads=2),
               dict(mm=2), dict(attn=3)):                                          # width % 16, head dim != 16, dtype
        bad = _desc(**kw)
        assert both(bad, io) == (-1, -1), kw
        assert prep(ref(bad), None) == -1, kw
        assert lib.cdseg_train_block_bytes(ref(bad), 10, 10, None, None, None, None) == -1, kw
    for i in (0, 5, 17):                                                           # a NULL / misaligned parameter
        for v in (None, ODD):
            bad = _desc()
            bad.param[i] = v
            assert both(bad, io) == (-1, -1) and prep(ref(bad), None) == -1, (i, v)
    bad = _desc(mm=1, attn=1)
    bad.shadow16[3] = ODD
    assert both(bad, io) == (-1, -1) and prep(ref(bad), None) == -1
    bad = _desc()
    bad.derived = None
    assert both(bad, io) == (-1, -1) and prep(ref(bad), None) == -1
    bad = _desc()
    bad.derived_bytes = _sizes(lib, bad, 0, 0)[2] - 256                            # a derived buffer that is too small
    assert both(bad, io) == (-1, -1) and prep(ref(bad), None) == -1
    for name in ("x_in", "x_conv", "tape", "scratch", "nbr", "gidx", "widx", "patch_start"):
        bad_io = _io()
        setattr(bad_io, name, None)
        assert both(d, bad_io) == (-1, -1), name
    bad_io = _io()
    bad_io.x_out = None
    assert fwd(ref(d), ref(bad_io), None) == -1
    for name in ("x_in", "x_conv", "tape", "scratch"):                             # misaligned rows
        bad_io = _io()
        setattr(bad_io, name, ODD)
        assert both(d, bad_io) == (-1, -1), name
    bad_io = _io()
    bad_io.x_out = ODD                                                             # (the backward does not read x_out)
    assert fwd(ref(d), ref(bad_io), None) == -1
    bad_io = _io()
    bad_io.mask1 = BUF + 2
    assert both(d, bad_io) == (-1, -1)
    bad_io = _io()
    bad_io.max_len = 1025                                                          # a patch holds at most 1024 slots
    assert both(d, bad_io) == (-1, -1)
    bad_io = _io()
    bad_io.t_rows = BUF                                                            # timestep rows without the scene offsets
    assert both(d, bad_io) == (-1, -1)
    tape, scratch = _sizes(lib, d, 100, 128)[:2]
    bad_io = _io()
    bad_io.tape_bytes = tape - 1
    assert both(d, bad_io) == (-1, -1)
    bad_io = _io()
    bad_io.scratch_bytes = scratch - 1
    assert both(d, bad_io) == (-1, -1)
    # the backward's own operands
    assert bwd(ref(d), ref(io), None, BUF, BUF, None, BUF, None) == -1
    assert bwd(ref(d), ref(io), BUF, None, BUF, None, BUF, None) == -1
    assert bwd(ref(d), ref(io), BUF, BUF, BUF, None, None, None) == -1
    assert bwd(ref(d), ref(io), ODD, BUF, BUF, None, BUF, None) == -1
    two = _io()
    two.x_conv = BUF + 4096
    assert bwd(ref(d), ref(two), BUF, BUF, None, None, BUF, None) == -1            # a distinct x_conv needs dx_conv
    # the row kernels
    assert lib.cdseg_residual(BUF, BUF, None, None, None, 0, BUF, 0, 32, None) == 0
    assert lib.cdseg_residual(None, BUF, None, None, None, 0, BUF, 5, 32, None) == -1
    assert lib.cdseg_residual(BUF, BUF, None, None, None, 0, BUF, 5, 30, None) == -1
    assert lib.cdseg_residual(ODD, BUF, None, None, None, 0, BUF, 5, 32, None) == -1
    assert lib.cdseg_residual(BUF, BUF, None, BUF, None, 2, BUF, 5, 32, None) == -1
    assert lib.cdseg_scale_cast(BUF, None, ODD, 1, 5, 32, None) == -1 and lib.cdseg_scale_cast(BUF, None, BUF, 2, 5, 32, None) == -1
    assert lib.cdseg_add_layernorm(BUF, None, None, BUF, BUF, 1e-5, BUF, BUF, 0, 5, 32, None) == -1
    assert lib.cdseg_add_layernorm(BUF, BUF, None, BUF, BUF, 1e-5, BUF, BUF, 0, 5, 4096, None) == -1
    assert lib.cdseg_gelu_fwd(BUF, None, 0, 64, None) == -1 and lib.cdseg_gelu_fwd(BUF, BUF, 0, 66, None) == -1
    assert lib.cdseg_gelu_bwd_cast(BUF, BUF, ODD, 1, 64, None) == -1 and lib.cdseg_gelu_bwd_cast(BUF, BUF, BUF, 1, 0, None) == 0


# ------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("c,heads,hidden", [(32, 2, 128), (64, 4, 256), (512, 32, 2048)])
def test_bytes_is_a_function_of_the_shape(c, heads, hidden):
    libs = {v: _lib.load(v) for v in _lib.VARIANTS}
    for mm, attn, det in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1)):
        prev = None
        for n in (1, 63, 64, 65, 200, 777, 5000, 120000):
            slots = (n + 63) // 64 * 64
            d = _desc(c, heads, hidden, mm, attn, det)
            got = {v: _sizes(lib, d, n, slots) for v, lib in libs.items()}
            assert got["bf16"] == got["f16"], (n, mm, attn)                       # the same in both builds
            s = got["bf16"]
            assert all(b % 256 == 0 and b > 0 for b in s), s
            assert _sizes(libs["bf16"], d, n, slots) == s                          # a function: asked twice, the same
            if prev is not None:
                assert all(a <= b for a, b in zip(prev, s)) and prev[0] < s[0], (prev, s)  # monotone in n
                assert prev[2] == s[2] and prev[3] == s[3]                         # weights do not depend on n
            prev = s
        # the 18 gradient views: ascending, apart, inside the slab, 256-byte aligned
        offs = (ctypes.c_size_t * 18)()
        assert libs["bf16"].cdseg_train_block_grad_offsets(ctypes.byref(d), offs) == 0
        offs = [int(o) for o in offs]
        numel = [c * 27 * c, c, c * c, c, c, c, c, c, 3 * c * c, 3 * c, c * c, c, c, c, hidden * c, hidden, c * hidden, c]
        ends = [o + 4 * k for o, k in zip(offs, numel)]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
        assert all(e <= o for e, o in zip(ends[:-1], offs[1:])) and ends[-1] <= prev[3]
        # the persistent derived buffer is about the size of the matrices (x2 under AMP: transposes and forward copies)
        mats = 4 * (27 * c * c + 5 * c * c + 2 * c * hidden)
        assert mats <= prev[2] <= mats + 12 * 256


# ------------------------------------------------------------------------------------------ the step on the emulated ops
def _mini(monkeypatch, emu_name="emu_block_ops"):
    import cdsegnet_amd.engine as engine
    import cdsegnet_amd.train_graph as tg
    from cdsegnet_amd import configs
    from cdsegnet_amd.param_init import fill_state_dict
    from cdsegnet_amd.registry import build_model
    import importlib
    emu_block_ops = importlib.import_module("tests." + emu_name)  # (the default: the emulated native Block and what it falls back to)
    from tests.helpers import load_fixture
    monkeypatch.setattr(engine, "ops", emu_block_ops)
    monkeypatch.setattr(tg, "ops", emu_block_ops)
    fx = load_fixture("train_step_mini.npz")
    cfg = configs.mini_config()
    cfg["backbone"]["enable_flash"] = False
    cfg["criteria"] = [dict(type="MSELoss", loss_weight=1.0, ignore_index=-1, batch_sample_point=-1),
                       dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                       dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)]
    model = build_model(cfg)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=int(fx["sd_seed"])))
    model.train()
    masks = {str(k): [fx[f"mask.{i}.{j}"] for j in range(int(fx["mask_counts"][i]))] for i, k in enumerate(fx["mask_names"])}
    draws = dict(ts=fx["ts"], noise=fx["noise"], perms=[list(p) for p in fx["perms"]], masks=masks)
    inp = {k: torch.as_tensor(fx[k]) for k in ("coord", "grid_coord", "feat", "offset", "segment")}
    return model, inp, draws, emu_block_ops


def test_native_step_on_the_emulated_ops_equals_the_autograd_step(monkeypatch):
    """The recorded mini step (tests/golden/train_step_mini.npz with its recorded masks) in both modes from the same state on
    the same emulation: the same 508 gradient names, the same loss and gradients up to fp32 rounding (metric and bound of the
    whole-step comparison in tests/test_gpu_deterministic.py: per tensor max |a - b| / (max |a| + 1e-3 top) < 1e-3; the loss
    within 1e-5); every Block is one forward and one backward call, a decoder's first Block reads an x_conv distinct from
    x_in, timestep rows enter the condition branch and their gradient reaches the timestep MLP; the real ops are never touched."""
    from cdsegnet_amd import models
    from cdsegnet_amd import ops as real_ops
    model, inp, draws, emu = _mini(monkeypatch)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls = {"fwd": [], "bwd": [], "gemm": 0}
    fwd, bwd, gemm = emu.train_block_forward, emu.train_block_backward, emu.E.gemm

    def c_fwd(tb, n, x_in, x_conv, t_rows, *a):
        calls["fwd"].append((x_conv is not x_in, t_rows is not None))
        return fwd(tb, n, x_in, x_conv, t_rows, *a)

    def c_bwd(*a):
        calls["bwd"].append(a[-3] is not None)  # dx_conv
        return bwd(*a)

    monkeypatch.setattr(emu, "train_block_forward", c_fwd)
    monkeypatch.setattr(emu, "train_block_backward", c_bwd)
    for name in ("train_block_forward", "train_block_backward", "train_block_prepare", "gemm", "layernorm"):
        monkeypatch.setattr(real_ops, name, lambda *a, **k: pytest.fail("the device ops were reached"))

    def run(mode):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        model.train_block = mode
        calls["fwd"], calls["bwd"] = [], []
        out = model(inp, draws={**draws, "masks": {k: list(v) for k, v in draws["masks"].items()}})
        out["loss"].backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        return float(out["loss"].detach()), grads, list(calls["fwd"]), list(calls["bwd"])

    l0, g0, f0, b0 = run("autograd")
    l1, g1, f1, b1 = run("native")
    blocks = sum(isinstance(m, models.Block) for m in model.modules())
    assert f0 == [] and b0 == []
    assert len(f1) == blocks and len(b1) == blocks and blocks > 0
    assert sum(xc for xc, _ in f1) == sum(b1) > 0      # the first Block behind every unpooling: a stale conv input
    assert 0 < sum(t for _, t in f1) < blocks          # the condition branch's Blocks take timestep rows, the others none
    assert set(g0) == set(g1) and len(g0) == 508
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    top = max(float(g.abs().max()) for g in g0.values())
    per = {k: float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0}
    worst = max(per, key=per.get)
    print(f"[measure] emulated step native vs autograd: loss {l0:.8f} / {l1:.8f}, worst gradient difference {per[worst]:.3e} ({worst})")
    assert per[worst] < 1e-3
    t_names = [k for k in g0 if "fc_t1" in k or "fc_t2" in k or "t_mlp" in k]
    assert t_names and all(float(g1[k].abs().max()) > 0 for k in t_names)


def test_prepare_runs_once_per_weight_version_on_the_emulation(monkeypatch):
    from cdsegnet_amd import models
    model, inp, draws, emu = _mini(monkeypatch)
    model.train_block = "native"
    blocks = sum(isinstance(m, models.Block) for m in model.modules())
    count = {"n": 0}
    prep = emu.train_block_prepare
    monkeypatch.setattr(emu, "train_block_prepare", lambda tb: (count.__setitem__("n", count["n"] + 1), prep(tb))[1])

    def fwd():
        return model(inp, draws={**draws, "masks": {k: list(v) for k, v in draws["masks"].items()}})["loss"]

    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    fwd()
    assert count["n"] == blocks
    fwd().backward()                       # a second forward without a step: the derived weights are current
    assert count["n"] == blocks
    opt.step()
    loss = fwd()
    assert count["n"] == 2 * blocks        # once per weight version
    opt.step()                             # an in-place weight change between forward and backward raises
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


@pytest.mark.parametrize("mode,emu_name", [("autograd", "emu_rows_ops"), ("native", "emu_block_ops")])
def test_deterministic_step_runs_on_the_emulated_ops_and_the_keyword_travels(monkeypatch, mode, emu_name):
    """`train_deterministic = True` on the emulated layer (autograd Blocks on tests/emu_rows_ops.py, whose `segment_sum` the
    deterministic gather backward needs; native Blocks on tests/emu_block_ops.py): every gradient reduction of the step (`linear_wgrad`, `conv_wgrad`,
    `layernorm_bwd`) receives `deterministic=True`, none of them receives the keyword in the default mode (ops.det_kw: the
    default call is what it was).  The keyword itself changes nothing here (a fixed-order torch sum is deterministic already),
    but the mode also takes the gather backward through `segment_sum`, another summation order: loss and gradients of the
    two modes agree by the metric and bound of the whole-step comparison above (1e-5 of the loss, 1e-3 per tensor)."""
    from tests import emu_ops
    model, inp, draws, emu = _mini(monkeypatch, emu_name)
    model.train_block = mode
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    seen = []

    def spy(name):
        fn = getattr(emu_ops, name)

        def wrapped(*a, **k):
            seen.append((name, k.get("deterministic", "absent")))
            return fn(*a, **k)
        monkeypatch.setattr(emu_ops, name, wrapped)

    for name in ("linear_wgrad", "conv_wgrad", "layernorm_bwd"):
        spy(name)

    def run(det):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        model.train_deterministic = det
        seen.clear()
        out = model(inp, draws={**draws, "masks": {k: list(v) for k, v in draws["masks"].items()}})
        out["loss"].backward()
        return float(out["loss"].detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}, list(seen)

    l0, g0, s0 = run(False)
    l1, g1, s1 = run(True)
    assert {n for n, _ in s0} == {n for n, _ in s1} == {"linear_wgrad", "conv_wgrad", "layernorm_bwd"}
    assert len(s0) == len(s1) and all(d == "absent" for _, d in s0) and all(d is True for _, d in s1)
    assert set(g0) == set(g1) and len(g1) == 508 and abs(l0 - l1) <= 1e-5 * abs(l0)
    top = max(float(g.abs().max()) for g in g0.values())
    per = {k: float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-3 * top) for k in g0}
    worst = max(per, key=per.get)
    print(f"[measure] emulated {mode} step, deterministic vs default: loss {l0:.8f} / {l1:.8f}, worst gradient difference "
          f"{per[worst]:.3e} ({worst})")
    assert per[worst] < 1e-3
