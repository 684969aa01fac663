"""CPU: which Block outputs the engine leaves unwritten (cdsegnet_amd.engine.block_outputs_read), the premise it rests on
(the pooling / un-pooling read the 16-bit copy alone), and the host-side chooser of the logits-in-tail kernel
(csrc/tail_outputs.h) compiled stand-alone."""
import ast
import inspect
import os
import shutil
import subprocess
import textwrap

import pytest

from cdsegnet_amd import configs, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP_PRECISIONS = ("bf16", "bf16+head", "fp16", "fp16+head")


def _blocks(cfg):
    """Every Block of a config as (branch, part, stage, stages of the branch's encoder, last of its stage)."""
    b = cfg["backbone"]
    out = []
    for branch in ("n", "c") if b["condition"] else ("n",):
        enc, dec = b[f"{branch}_enc_depths"], b[f"{branch}_dec_depths"]
        assert len(dec) == len(enc) - 1
        for part, depths in (("enc", enc), ("dec", dec)):
            for s, depth in enumerate(depths):
                out += [(branch, part, s, len(enc), i == depth - 1) for i in range(depth)]
    return out


CONFIGS = [(ds, variant) for ds in ("scannet", "scannet200", "nuscenes") for variant in ("CDSegNet", "PTv3")]


@pytest.mark.parametrize("dataset,variant", CONFIGS)
@pytest.mark.parametrize("precision", LP_PRECISIONS)
def test_exactly_the_named_blocks_lose_an_output(dataset, variant, precision):
    cfg = configs.model_config(dataset, variant)
    assert cfg["backbone"]["condition"] == (variant == "CDSegNet")
    blocks = _blocks(cfg)
    got = {blk: engine.block_outputs_read(blk[1], blk[2], blk[3], blk[4], precision, branch=blk[0]) for blk in blocks}
    x_dead = {blk for blk, (x, xc) in got.items() if not x}
    xc_dead = {blk for blk, (x, xc) in got.items() if not xc}
    want_x = set()
    for branch, part, s, ns, last in blocks:
        if not last:
            continue
        if part == "enc" and s < ns - 1:  # every encoder stage but the bottleneck, both branches
            want_x.add((branch, part, s, ns, last))
        if part == "dec" and s > 0:       # every decoder stage but the last, both branches
            want_x.add((branch, part, s, ns, last))
    last_n = ("n", "dec", 0, len(cfg["backbone"]["n_enc_depths"]), True)
    if precision.endswith("+head"):
        want_xc = {last_n}  # the fp32 head reads the fp32 rows
    else:
        want_xc = set()
        want_x.add(last_n)  # a 16-bit head reads the 16-bit copy
    assert x_dead == want_x and xc_dead == want_xc
    assert all(x or xc for x, xc in got.values()), "a Block nobody reads"
    # the bottlenecks (cross block, multi-step hoist, trace) and the c-branch's last decoder Block (c-head) stay live
    for branch, part, s, ns, last in blocks:
        if (part == "enc" and s == ns - 1) or (branch == "c" and part == "dec" and s == 0):
            assert got[(branch, part, s, ns, last)] == (True, True)


@pytest.mark.parametrize("dataset,variant", CONFIGS)
def test_everything_is_read_in_fp32_on_the_binding_path_and_under_the_saturation_diagnostic(dataset, variant):
    blocks = _blocks(configs.model_config(dataset, variant))
    for branch, part, s, ns, last in blocks:
        for precision in ("fp32", "fp32x3"):
            assert engine.block_outputs_read(part, s, ns, last, precision, branch=branch) == (True, True)
        for precision in LP_PRECISIONS:
            assert engine.block_outputs_read(part, s, ns, last, precision, branch=branch, diagnostic=True) == (True, True)
            assert engine.block_outputs_read(part, s, ns, last, precision, branch=branch, native=False) == (True, True)
    # a model without a seg head returns the last Block's rows themselves
    assert engine.block_outputs_read("dec", 0, 5, True, "fp16+head", has_head=False) == (True, True)


def test_run_block_keeps_everything_live_by_default():
    sig = inspect.signature(engine.Engine.run_block)
    assert sig.parameters["live"].default == (True, True) and sig.parameters["head"].default is None
    assert engine.LOGITS_IN_TAIL_MIN_ROWS >= 65_536


@pytest.mark.parametrize("fn,incoming", [("run_pooling", {"st"}), ("run_unpooling", {"st", "parent"})])
def test_pooling_and_unpooling_read_only_the_16_bit_copy_of_the_incoming_state(fn, incoming):
    """The premise of a dead x: what follows a stage's last Block never touches the incoming State's fp32 rows."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(getattr(engine.Engine, fn))))
    seen = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in incoming:
            seen.setdefault(node.value.id, set()).add(node.attr)
    assert set(seen) == incoming
    for name, attrs in seen.items():
        assert "xc" in attrs and "x" not in attrs, f"{fn} reads {name}.x"
        assert attrs <= {"xc", "level", "curves", "parent"}, (fn, name, attrs)


MAIN = r"""
#include <cstdio>
#include "cdsegnet_amd/csrc/tail_outputs.h"
int main() {
  alignas(16) static float logits[64]; static float w[64]; static int idx[4];
  int bad = 0;
  auto expect = [&](int got, int want, const char* what) { if (got != want) { std::printf("%s: %d != %d\n", what, got, want); ++bad; } };
  // the LDS budget: the C = 64 tail leaves 6 144 B of the 80 KB that keep two workgroups on a CU
  expect(tail_rr_lds_bytes(64), 75776, "tail LDS at C = 64");
  expect(TAIL_RR_LDS_TWO_PER_CU - tail_rr_lds_bytes(64), 6144, "left at C = 64");
  expect(tail_logits_lds_bytes(64, 20), 20 * 68 * 4 + 80, "head LDS, 20 classes");
  for (int k = 1; k <= 256; ++k) {
    const bool fits = tail_rr_lds_bytes(64) + tail_logits_lds_bytes(64, k) <= TAIL_RR_LDS_TWO_PER_CU;
    const int want = (k % 4 == 0 && k <= 20) ? CDSEG_OK : CDSEG_ERR_UNSUPPORTED;
    if (fits != (k <= 22)) { std::printf("LDS rule at %d classes\n", k); ++bad; }
    expect(tail_logits_status(64, k, k, logits, w, nullptr), want, "classes at C = 64");
  }
  expect(tail_logits_status(64, 20, 20, logits, w, idx), CDSEG_OK, "with out_idx");
  expect(tail_logits_status(64, 20, 24, logits, w, nullptr), CDSEG_OK, "padded rows");
  expect(tail_logits_status(64, 20, 22, logits, w, nullptr), CDSEG_ERR_UNSUPPORTED, "ld % 4");
  expect(tail_logits_status(64, 20, 16, logits, w, nullptr), CDSEG_ERR_UNSUPPORTED, "ld < classes");
  expect(tail_logits_status(64, 20, 20, logits + 1, w, nullptr), CDSEG_ERR_UNSUPPORTED, "unaligned logits");
  expect(tail_logits_status(32, 16, 16, logits, w, nullptr), CDSEG_ERR_UNSUPPORTED, "C = 32");
  expect(tail_logits_status(128, 16, 16, logits, w, nullptr), CDSEG_ERR_UNSUPPORTED, "C = 128");
  expect(tail_logits_status(64, 20, 20, nullptr, w, nullptr), CDSEG_ERR_ARG, "no logits");
  expect(tail_logits_status(64, 20, 20, logits, nullptr, nullptr), CDSEG_ERR_ARG, "no weights");
  expect(tail_logits_status(64, 0, 20, logits, w, nullptr), CDSEG_ERR_ARG, "no classes");
  std::printf("bad = %d\n", bad);
  return bad ? 1 : 0;
}
"""


def test_the_chooser_compiled_stand_alone(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "chooser.cpp", tmp_path / "chooser"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", ROOT, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
