"""GPU: the AMP training step (`DefaultSegmentorV2.train_precision = "fp16-amp" | "bf16-amp"`): every trunk Linear and sparse
conv on 16-bit products (cdseg_gemm on 16-bit operands, cdseg_linear_wgrad16 / cdseg_conv_wgrad16) next to the 16-bit
attention core, both builds of the library.  tests/test_gpu_wgrad16.py pins the weight gradient's arithmetic; this file pins
the autograd functions (exactly, on integers), the routing of a whole step, the GradScaler behaviour and the saved
activations.
"""
import threading

import numpy as np
import pytest
import torch

from cdsegnet_amd import ops as O
from cdsegnet_amd import train_graph as TG
from tests.helpers import load_fixture
from tests.test_gpu_attention_bwd16 import _draws, _inp, _mini_model
from tests.test_gpu_ops import LP, _library_variant, _physical, dev, ops, report  # noqa: F401  (fixtures: lp="f16" -> the half build)

pytestmark = pytest.mark.gpu

LPS = pytest.mark.parametrize("lp", ["bf16", "f16"])
TPS = pytest.mark.parametrize("tp,lp", [("bf16-amp", "bf16"), ("fp16-amp", "f16")])
PLANS = pytest.mark.parametrize("flash", [False, True], ids=["padded", "flash"])
LOSS_CAP = {"fp16-amp": 0.012, "bf16-amp": 0.04}  # tests/test_gpu_e2e.py's whole-trunk 16-bit logit bounds (sanity cap)


def _ints(rng, *shape):
    return torch.as_tensor(rng.integers(-3, 4, size=shape)).double().cuda()


def _same(got, want):
    """fp32 result == the integer result (fp64 on small integers is exact)."""
    return got.dtype == torch.float32 and bool((got.double() == want).all())


# ------------------------------------------------------------------------------------------ the autograd functions alone
@LPS
def test_linear16_function_is_exact_on_integers(ops, lp):
    rng = np.random.default_rng(1)
    M, K, N = 37, 16, 48
    x, w, b, dy = _ints(rng, M, K), _ints(rng, N, K), _ints(rng, N), _ints(rng, M, N)
    xf, wf, bf = (t.float().requires_grad_(True) for t in (x, w, b))
    y = TG._Linear16.apply(xf, wf, bf, lp)
    y.backward(dy.float())
    torch.cuda.synchronize()
    assert _same(y.detach(), x @ w.T + b)
    assert _same(xf.grad, dy @ w) and _same(wf.grad, dy.T @ x) and _same(bf.grad, dy.sum(0))


@LPS
def test_subm_conv16_function_is_exact_on_integers(ops, lp):
    fx = load_fixture("serialization_room1500.npz")
    zs, perm0, g0, b0, depth, p = _physical(ops, fx)
    nbr = ops.nbr_table(zs, g0, b0, depth, 3, True).contiguous()
    kvol, M = nbr.shape
    C = 32
    rng = np.random.default_rng(2)
    x, w5, b, dy = _ints(rng, M, C), _ints(rng, C, 3, 3, 3, C), _ints(rng, C), _ints(rng, M, C)
    w3 = w5.reshape(C, kvol, C)
    y64 = b.expand(M, C).clone()
    dx64, dw64 = torch.zeros_like(x), torch.zeros_like(w3)
    for o in range(kvol):
        rows = (nbr[o] >= 0).nonzero().flatten()
        src = nbr[o][rows].long()
        y64[rows] += x[src] @ w3[:, o].T
        dx64.index_add_(0, src, dy[rows] @ w3[:, o])
        dw64[:, o] = dy[rows].T @ x[src]
    xf, wf, bf = (t.float().requires_grad_(True) for t in (x, w5, b))
    y = TG._SubMConv16.apply(xf, wf, bf, nbr, lp)
    y.backward(dy.float())
    torch.cuda.synchronize()
    assert _same(y.detach(), y64)
    assert _same(xf.grad, dx64) and _same(wf.grad.reshape(C, kvol, C), dw64) and _same(bf.grad, dy.sum(0))


# ------------------------------------------------------------------------------------------ the whole step
class _Calls:
    """Wraps the ops the training graph launches its products through (it calls them through the module): kind and operand
    dtypes of every launch."""

    NAMES = ("gemm", "linear_wgrad", "conv_wgrad", "attention", "attention_bwd")

    def __init__(self, monkeypatch):
        self.log = []
        self.lock = threading.Lock()  # (autograd runs backward on a thread of its own)
        for name in self.NAMES:
            monkeypatch.setattr(O, name, self._wrap(name, getattr(O, name)))

    def _wrap(self, name, fn):
        def call(a, b, *args, **kw):
            dts = (a.dtype, (args[0] if name == "conv_wgrad" else b).dtype)  # conv_wgrad(x, nbr, dy, ...)
            with self.lock:
                self.log.append((name, dts))
            return fn(a, b, *args, **kw)
        return call

    def counts(self, dtype):
        """Every launch has both operands of `dtype`; -> launches per kind, and clears the log."""
        bad = {(n, d) for n, d in self.log if d != (dtype, dtype)}
        assert self.log and not bad, bad
        out = {n: sum(k == n for k, _ in self.log) for n in self.NAMES}
        self.log.clear()
        return out


@TPS
@PLANS
def test_step_routes_every_product_through_16_bit_kernels(ops, monkeypatch, tp, lp, flash):
    """Forward + backward in the new modes: every GEMM, weight-gradient and attention launch has 16-bit operands of the chosen
    type, none is fp32, and there are as many as in the fp32 step on the same draws; fp32 finite loss; finite gradients on
    the fp32 step's parameters.  Padded plan (the fixture's): the loss within the sanity cap of the recorded fp32 loss,
    distances to the recorded step reported, and "fp32" afterwards reproduces the fixture's loss."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    calls = _Calls(monkeypatch)
    inp = _inp(fx)
    model.zero_grad()
    model(inp, draws=_draws(fx))["loss"].backward()
    torch.cuda.synchronize()
    n32 = calls.counts(torch.float32)
    have32 = {k for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    assert "train_precision" not in model.state_dict()
    model.train_precision = tp
    loss = model(inp, draws=_draws(fx))["loss"]
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    torch.cuda.synchronize()
    n16 = calls.counts(LP())
    assert n16 == n32 and min(n16.values()) > 0, (n16, n32)
    named = dict(model.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == have32
    assert all(bool(torch.isfinite(p.grad).all()) for p in named.values() if p.grad is not None)
    if not flash:
        e_loss = abs(float(loss.detach()) - float(fx["loss"]))
        names = [str(n) for n in fx["grad_names"]]
        gn = np.array([float(named[k].grad.norm()) for k in names])
        ref = fx["grad_norms"]
        rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
        cos = 1.0
        for k in fx.files:
            if k.startswith("g."):
                a, b = named[k[2:]].grad.cpu().double().flatten(), torch.as_tensor(fx[k]).double().flatten()
                cos = min(cos, float(a @ b / (a.norm() * b.norm())))
        report(f"train step {tp} vs the reference's recorded fp32 step", launches=sum(n16.values()), loss_diff=e_loss,
               worst_grad_norm_rel=float(rel.max()), min_cosine_of_8_full_grads=cos)
        assert e_loss < LOSS_CAP[tp], e_loss
        model.zero_grad()
        model.train_precision = "fp32"
        l32 = float(model(inp, draws=_draws(fx))["loss"].detach())
        assert abs(l32 - float(fx["loss"])) < 1e-4
    else:
        report(f"train step {tp} flash plan", launches=sum(n16.values()), loss=float(loss.detach()))


@TPS
@PLANS
def test_reference_run_step_with_amp_and_grad_scaler(ops, tp, lp, flash):
    """The reference trainer's run_step (engines/train.py:216-271) with cfg.enable_amp = True.  bfloat16: the scaler finds no
    overflow and the parameters move.  Half: each step either finds no overflow (scale unchanged, parameters move) or is
    skipped (scale halved, every parameter bit-identical) - a skipped step proves that an inf reaches .grad through the
    unsaturated cast of dy; within 17 steps (65536 -> 1) one must move the parameters."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    model.train_precision = tp
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    scaler = torch.cuda.amp.GradScaler()
    inp = _inp(fx)
    skipped, moved = 0, 0.0
    for _ in range(17):
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        with torch.cuda.amp.autocast(enabled=True):
            loss = model(inp, draws=_draws(fx))["loss"]
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scale = scaler.get_scale()
        scaler.update()
        torch.cuda.synchronize()
        if scaler.get_scale() == scale:
            moved = max(float((p.detach() - before[k]).abs().max()) for k, p in model.named_parameters())
            break
        assert tp == "fp16-amp", "the scaler found an overflow in bfloat16"
        assert scaler.get_scale() == scale / 2
        assert all(torch.equal(p.detach(), before[k]) for k, p in model.named_parameters()), "a skipped step moved parameters"
        skipped += 1
    report(f"run_step {tp} {'flash' if flash else 'padded'}", loss=float(loss.detach()), skipped_steps=skipped,
           final_scale=scaler.get_scale(), max_param_move=moved)
    assert moved > 1e-5


@TPS
@PLANS
def test_four_steps_on_one_batch_descend(ops, tp, lp, flash):
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), flash)
    model.train_precision = tp
    opt = torch.optim.AdamW(model.parameters(), lr=0.002, weight_decay=0.05)
    inp = _inp(fx)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = model(inp, draws=_draws(fx))["loss"]
        loss.backward()
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
        losses.append(float(loss.detach()))
        opt.step()
    torch.cuda.synchronize()
    report(f"4 steps {tp} {'flash' if flash else 'padded'}", l0=losses[0], l1=losses[1], l2=losses[2], l3=losses[3])
    assert np.isfinite(losses).all() and all(b < a for a, b in zip(losses, losses[1:])), losses


@TPS
def test_saved_inputs_of_linears_and_convs_are_16_bit(ops, monkeypatch, tp, lp):
    """One forward under torch.autograd.graph.saved_tensors_hooks: the A operand of every forward GEMM (the input of a Linear /
    sparse conv function) is a tensor the graph saves; in the new modes those are 16-bit tensors and their bytes are half the
    fp32 step's."""
    fx = load_fixture("train_step_mini.npz")
    model, _ = _mini_model(fx, torch.device("cuda"), False)
    inp = _inp(fx)

    def saved_input_bytes(precision, dtype):
        model.train_precision = precision
        inputs, packed = [], {}
        gemm = O.gemm

        def logged(a, *args, **kw):
            inputs.append(a)
            return gemm(a, *args, **kw)

        def pack(t):
            packed[t.data_ptr()] = t.dtype
            return t

        with monkeypatch.context() as mp, torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            mp.setattr(O, "gemm", logged)
            out = model(inp, draws=_draws(fx))
        assert inputs and all(a.dtype == dtype and packed.get(a.data_ptr()) == dtype for a in inputs)
        del out
        return sum(a.numel() * a.element_size() for a in inputs), len(inputs)

    b32, n32 = saved_input_bytes("fp32", torch.float32)
    b16, n16 = saved_input_bytes(tp, LP())
    report(f"saved Linear / conv inputs {tp}", fp32_bytes=b32, amp_bytes=b16, functions=n16)
    assert n16 == n32 and 2 * b16 == b32
