"""CPU: the fused optimizer step's host side - argument checks of the entry points (before any launch or copy, so they run
without a GPU), the chunk list against a Python restatement, FusedAdamW's constructor, state_dict exchange with
torch.optim.AdamW, the registry hook and the shadow-copy lookup."""
import ctypes
import os

import pytest
import torch

from cdsegnet_amd import _lib
from cdsegnet_amd import optim as OPT
from cdsegnet_amd.optim import FusedAdamW

OK, ERR_ARG, ERR_WS, ERR_UNSUP = 0, -1, -3, -4
CHUNK = 8192  # CDSEG_OPT_CHUNK
P = 0x10000   # a non-null, 16-byte aligned address that is never dereferenced: every check below fails before a launch


@pytest.fixture(scope="module", params=_lib.VARIANTS)
def lib(request):
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.LIB_PATH_F16)):
        from cdsegnet_amd.build import build_library
        build_library()
    return _lib.load(request.param)


def _table(count=2, **over):
    t = (_lib.OptTensor * count)()
    for i, e in enumerate(t):
        e.p, e.g, e.m, e.v, e.p16, e.step = P, P, P, P, None, P
        e.n, e.group, e.flags = 1000 + i, i % 2, _lib.OPT_CLIP
    for k, v in over.items():
        setattr(t[count - 1], k, v)
    return t


def _groups(n=2, **over):
    g = (_lib.OptGroup * n)()
    for e in g:
        e.lr, e.beta1, e.beta2, e.eps, e.weight_decay = 2e-3, 0.9, 0.999, 1e-8, 0.05
    for k, v in over.items():
        setattr(g[n - 1], k, v)
    return g


def test_header_constant_matches():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cdseg.h")).read()
    assert f"#define CDSEG_OPT_CHUNK {CHUNK}\n" in hdr
    assert ctypes.sizeof(_lib.OptTensor) == 64 and ctypes.sizeof(_lib.OptGroup) == 40


def test_entry_points_check_their_arguments_before_any_launch(lib):
    nch = 2  # two tensors below one chunk each
    ws = lib.cdseg_opt_ws_bytes(2, nch)
    assert ws > 0 and lib.cdseg_opt_ws_bytes(0, nch) == 0 and lib.cdseg_opt_ws_bytes(2, 0) == 0

    def norm(**k):
        a = dict(tab=_table(), count=2, chunks=P, nch=nch, scale=None, max_norm=1.0, out=P, ws=P, ws_bytes=ws)
        a.update(k)
        return lib.cdseg_grad_norm(a["tab"], a["count"], a["chunks"], a["nch"], a["scale"], a["max_norm"], a["out"], a["ws"],
                                   a["ws_bytes"], None)

    def step(**k):
        a = dict(tab=_table(), count=2, groups=_groups(), ng=2, chunks=P, nch=nch, scale=None, found=None, coef=None, ws=P,
                 ws_bytes=ws)
        a.update(k)
        return lib.cdseg_adamw_step(a["tab"], a["count"], a["groups"], a["ng"], a["chunks"], a["nch"], a["scale"], a["found"],
                                    a["coef"], a["ws"], a["ws_bytes"], None)

    for call in (norm, step):
        for field in ("p", "g", "m", "v", "step"):
            assert call(tab=_table(**{field: None})) == ERR_ARG, field       # NULL
            assert call(tab=_table(**{field: P + 2})) == ERR_ARG, field      # not 4-byte aligned
        assert call(tab=_table(p16=P + 1)) == ERR_ARG
        assert call(tab=None) == ERR_ARG and call(count=0) == ERR_ARG and call(count=-1) == ERR_ARG
        assert call(tab=_table(n=0)) == ERR_ARG and call(tab=_table(n=-5)) == ERR_ARG
        assert call(tab=_table(n=1 << 31)) == ERR_UNSUP
        assert call(tab=_table(flags=4)) == ERR_ARG
        assert call(chunks=None) == ERR_ARG and call(chunks=P + 2) == ERR_ARG
        assert call(nch=nch + 1) == ERR_ARG and call(tab=_table(n=CHUNK + 1)) == ERR_ARG   # not the table's chunk count
        assert call(ws=None) == ERR_WS and call(ws_bytes=ws - 1) == ERR_WS and call(ws_bytes=0) == ERR_WS
        assert call(ws=P + 8) == ERR_ARG                                                     # misaligned workspace
        assert call(scale=P + 2) == ERR_ARG
    assert norm(out=None) == ERR_ARG and norm(out=P + 1) == ERR_ARG and norm(max_norm=-1.0) == ERR_ARG
    assert norm(max_norm=float("nan")) == ERR_ARG
    assert step(tab=_table(group=2)) == ERR_ARG and step(tab=_table(group=-1)) == ERR_ARG   # group index out of range
    assert step(groups=None) == ERR_ARG and step(ng=0) == ERR_ARG
    assert step(groups=_groups(17), ng=17) == ERR_UNSUP
    assert step(groups=_groups(beta2=1.0)) == ERR_ARG and step(groups=_groups(lr=-1.0)) == ERR_ARG
    assert step(groups=_groups(eps=float("nan"))) == ERR_ARG
    assert step(found=P + 2) == ERR_ARG and step(coef=P + 1) == ERR_ARG


def _chunks_py(sizes):
    return [(i, s) for i, n in enumerate(sizes) for s in range(0, n, CHUNK)]


def test_chunk_list_equals_the_python_restatement_and_covers_every_element_once(lib):
    sizes = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7]
    arr = (ctypes.c_long * len(sizes))(*sizes)
    n = ctypes.c_long()
    assert lib.cdseg_opt_chunks(arr, len(sizes), None, ctypes.byref(n)) == OK
    want = _chunks_py(sizes)
    assert n.value == len(want) == 1 + 1 + 1 + 2 + 4
    out = (ctypes.c_int32 * (2 * n.value))()
    assert lib.cdseg_opt_chunks(arr, len(sizes), out, ctypes.byref(n)) == OK
    got = [(out[2 * k], out[2 * k + 1]) for k in range(n.value)]
    assert got == want and got == sorted(got)                       # tensors and offsets ascend
    cover = [[0] * s for s in sizes]
    for t, s in got:
        for e in range(s, min(s + CHUNK, sizes[t])):
            cover[t][e] += 1
    assert all(c == 1 for row in cover for c in row)                # every element exactly once
    assert lib.cdseg_opt_chunks(None, 1, None, ctypes.byref(n)) == ERR_ARG
    assert lib.cdseg_opt_chunks(arr, 0, None, ctypes.byref(n)) == ERR_ARG
    assert lib.cdseg_opt_chunks(arr, len(sizes), None, None) == ERR_ARG
    assert lib.cdseg_opt_chunks((ctypes.c_long * 1)(0), 1, None, ctypes.byref(n)) == ERR_ARG
    assert lib.cdseg_opt_chunks((ctypes.c_long * 1)(1 << 31), 1, None, ctypes.byref(n)) == ERR_UNSUP


def _toy():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.GELU(), torch.nn.Linear(7, 3))


def test_constructor_rejections():
    m = _toy()
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(NotImplementedError, match="amsgrad"):
            FusedAdamW(m.parameters(), lr=1e-3, **kw)
    with pytest.raises(NotImplementedError, match="fp32"):
        FusedAdamW([torch.zeros(4, dtype=torch.float64, requires_grad=True)], lr=1e-3)
    with pytest.raises(NotImplementedError, match="fp32"):
        FusedAdamW([torch.zeros(4, dtype=torch.bfloat16, requires_grad=True)], lr=1e-3)
    with pytest.raises(NotImplementedError, match="tensor lr"):
        FusedAdamW(m.parameters(), lr=torch.tensor(1e-3))
    for kw in (dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(max_grad_norm=-1.0),
               dict(shadow16="fp8"), dict(clip_params=[torch.zeros(3)], max_grad_norm=1.0)):
        with pytest.raises(ValueError):
            FusedAdamW(m.parameters(), **kw)
    with pytest.raises(_lib.CdsegError):  # the 16-bit copies are made by the library's cast: no CPU form
        FusedAdamW(m.parameters(), lr=1e-3, shadow16="f16")
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    with pytest.raises(NotImplementedError, match="fixed at construction"):
        opt.add_param_group(dict(params=[torch.zeros(3, requires_grad=True)]))
    m(torch.randn(2, 5)).sum().backward()
    with pytest.raises(_lib.CdsegError, match="GPU only"):  # CPU parameters: loud at step, never a torch fallback
        opt.step()
    assert opt._step_supports_amp_scaling is True


def test_state_dict_round_trips_with_torch_adamw():
    m = _toy()
    blk, rest = list(m[0].parameters()), list(m[2].parameters())
    groups = lambda: [dict(params=rest, lr=0.002), dict(params=blk, lr=0.0002)]  # noqa: E731
    ref = torch.optim.AdamW(groups(), lr=0.002, weight_decay=0.05)
    for _ in range(2):
        ref.zero_grad()
        m(torch.randn(4, 5)).square().sum().backward()
        ref.step()
    sd = ref.state_dict()
    opt = FusedAdamW(groups(), lr=0.002, weight_decay=0.05)
    assert opt.state_dict()["state"] == {} and opt.state_dict()["param_groups"][0].keys() == sd["param_groups"][0].keys()
    opt.load_state_dict(sd)
    for p in m.parameters():
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 2.0 and st["step"].shape == ()
        assert st["exp_avg"].shape == p.shape and torch.equal(st["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
        # the loaded moments live in the optimizer's flat buffers
        assert st["exp_avg"].untyped_storage().data_ptr() == opt._m.untyped_storage().data_ptr()
        assert st["exp_avg_sq"].untyped_storage().data_ptr() == opt._v.untyped_storage().data_ptr()
        assert st["exp_avg"].data_ptr() % 16 == 0
    assert [g["lr"] for g in opt.param_groups] == [0.002, 0.0002]
    back = torch.optim.AdamW(groups(), lr=0.1)
    back.load_state_dict(opt.state_dict())
    assert [g["lr"] for g in back.param_groups] == [0.002, 0.0002] and back.param_groups[0]["weight_decay"] == 0.05
    for p in m.parameters():
        assert float(back.state[p]["step"]) == 2.0
        assert torch.equal(back.state[p]["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(back.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    ref.zero_grad()
    m(torch.randn(4, 5)).square().sum().backward()
    back.step()  # torch's optimizer runs on the state that went through FusedAdamW
    assert float(back.state[blk[0]]["step"]) == 3.0
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[0.002, 0.0002], total_steps=10)  # schedulers take it as an Optimizer
    assert sched.get_last_lr()[0] < 0.002


def test_register_optimizers_into_a_pointcept_style_registry():
    from cdsegnet_amd import pointcept_plugin as plug
    from cdsegnet_amd.registry import Registry
    reg = plug.register_optimizers(Registry("optimizers"))
    assert reg.get("FusedAdamW") is FusedAdamW
    m = _toy()
    opt = reg.build(dict(type="FusedAdamW", lr=0.002, weight_decay=0.05), default_args=dict(params=m.parameters()))
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.Optimizer) and opt.param_groups[0]["weight_decay"] == 0.05


def test_shadow16_lookup_refuses_stale_foreign_and_mistyped_tensors():
    w = torch.randn(6, 4)
    OPT.register_shadow(w, w.to(torch.float16))
    s = OPT.shadow16(w, torch.float16)
    assert s is not None and s.dtype == torch.float16 and torch.equal(s, w.to(torch.float16))
    assert OPT.shadow16(w.detach(), torch.float16) is s           # same storage, shape, version: what a Function's forward sees
    assert OPT.shadow16(w, torch.bfloat16) is None                # wrong dtype
    assert OPT.shadow16(torch.randn(6, 4), torch.float16) is None  # a foreign tensor
    assert OPT.shadow16(w.view(4, 6), torch.float16) is None       # same storage, another shape
    assert OPT.shadow16(w[1:], torch.float16) is None
    w.add_(1.0)                                                    # an in-place change moves _version: stale
    assert OPT.shadow16(w, torch.float16) is None
    OPT.register_shadow(w, w.to(torch.float16))
    assert OPT.shadow16(w, torch.float16) is not None
    w.data.mul_(2.0)  # the documented limitation: .data does not move _version, the stale copy is still handed out
    assert OPT.shadow16(w, torch.float16) is not None
    with pytest.raises(ValueError):
        OPT.register_shadow(w, w.to(torch.float16)[1:])
    with pytest.raises(ValueError):
        OPT.register_shadow(w, w.clone())
    key = w.data_ptr()
    alias = w.data                                                 # a second tensor object on the same storage registers ...
    OPT.register_shadow(alias, alias.to(torch.float16))
    del w, s
    assert key in OPT._SHADOWS and OPT.shadow16(alias, torch.float16) is not None  # ... and survives the first object
    del alias
    assert key not in OPT._SHADOWS                                 # dropped with the object that registered it last
