"""The CPU emulations of the op layer (tests/emu_*.py) against cdsegnet_amd.ops, by signature: every public function an
emulation module defines itself (not one reached through its `__getattr__` fallback) exists in `ops` with the same
positional parameters (names, order, kinds, defaults) and the same set of keyword-only (name, default) pairs, and every
module-level integer constant equals the one in `ops`.  No allow-list: an emulation follows the real op, never the reverse.
(What the emulations COMPUTE is held to the kernels in tests/test_gpu_emu_conformance.py.)"""
import importlib
import inspect
import types

import pytest

from cdsegnet_amd import ops

EMU_MODULES = ("emu_ops", "emu_norm_ops", "emu_block_ops", "emu_rows_ops", "emu_fusion_ops", "emu_skip_ops", "emu_select_ops")
_POSITIONAL = (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.VAR_POSITIONAL)


def emulated_functions(module_name):
    """{name: function} of the public functions defined in tests/<module_name>.py itself."""
    mod = importlib.import_module("tests." + module_name)
    return {name: f for name, f in vars(mod).items()
            if not name.startswith("_") and isinstance(f, types.FunctionType) and f.__module__ == mod.__name__}


def emulated_constants(module_name):
    """{name: value} of the module-level integers and tuples of integers of tests/<module_name>.py."""
    mod = importlib.import_module("tests." + module_name)

    def is_int(v):
        return isinstance(v, int) and not isinstance(v, bool)

    return {name: v for name, v in vars(mod).items() if not name.startswith("_")
            and (is_int(v) or (isinstance(v, tuple) and len(v) and all(is_int(e) for e in v)))}


def signature_parts(fn):
    """(positional parameters as (name, kind, default), the set of keyword-only (name, default), has **kwargs)."""
    params = inspect.signature(fn).parameters.values()
    pos = [(p.name, p.kind, p.default) for p in params if p.kind in _POSITIONAL]
    kwo = {(p.name, repr(p.default)) for p in params if p.kind == inspect.Parameter.KEYWORD_ONLY}
    return pos, kwo, any(p.kind == inspect.Parameter.VAR_KEYWORD for p in params)


def signature_difference(emu_fn, real_fn):
    """None when the two agree by the rule of this file, else a sentence saying where they do not."""
    (pe, ke, ve), (pr, kr, vr) = signature_parts(emu_fn), signature_parts(real_fn)
    if pe != pr:
        return f"positional parameters differ: emulation {inspect.signature(emu_fn)} vs ops {inspect.signature(real_fn)}"
    if ke != kr:
        return f"keyword-only parameters differ: only in the emulation {sorted(ke - kr)}, only in ops {sorted(kr - ke)}"
    if ve != vr:
        return "one of the two takes **kwargs, the other does not"
    return None


CASES = [(m, name) for m in EMU_MODULES for name in sorted(emulated_functions(m))]


def test_the_enumeration_sees_the_emulations():
    """The walk finds what it is meant to: the seven modules, the large one whole, and not the fallbacks."""
    names = {m: set(emulated_functions(m)) for m in EMU_MODULES}
    assert len(names["emu_ops"]) >= 77 and {"gemm", "randn", "knn1", "pool_level"} <= names["emu_ops"]
    assert "gemm" not in names["emu_norm_ops"] and "segment_max_arg" in names["emu_norm_ops"]
    assert {"train_block_forward", "train_block_backward", "residual"} <= names["emu_block_ops"]
    assert names["emu_rows_ops"] == {"segment_sum"} and names["emu_select_ops"] == {"slots_select"}
    assert {"ACT_GELU", "F32", "BF16", "ATTN_Q_PRESCALED", "DEEP_CHANNELS"} <= set(emulated_constants("emu_ops"))
    assert {"TB_PARAMS", "TB_MATRICES"} <= set(emulated_constants("emu_block_ops"))


@pytest.mark.parametrize("module_name,name", CASES, ids=[f"{m}.{n}" for m, n in CASES])
def test_emulated_function_has_the_signature_of_the_real_op(module_name, name):
    real = getattr(ops, name, None)
    assert isinstance(real, types.FunctionType), f"cdsegnet_amd.ops has no function {name}"
    diff = signature_difference(emulated_functions(module_name)[name], real)
    assert diff is None, f"tests/{module_name}.py {name}: {diff}"


@pytest.mark.parametrize("module_name", EMU_MODULES)
def test_emulated_constants_equal_the_real_ones(module_name):
    for name, value in emulated_constants(module_name).items():
        assert hasattr(ops, name), f"cdsegnet_amd.ops has no constant {name} (tests/{module_name}.py defines it)"
        assert getattr(ops, name) == value, f"{name}: tests/{module_name}.py has {value}, ops has {getattr(ops, name)}"


def test_emulated_classes_are_built_like_the_real_ones():
    """A class an emulation defines (the training Block's descriptor) is constructed with the real one's arguments."""
    for m in EMU_MODULES:
        mod = importlib.import_module("tests." + m)
        for name, cls in vars(mod).items():
            if isinstance(cls, type) and cls.__module__ == mod.__name__ and not name.startswith("_"):
                assert isinstance(getattr(ops, name, None), type), f"cdsegnet_amd.ops has no class {name}"
                diff = signature_difference(cls.__init__, getattr(ops, name).__init__)
                assert diff is None, f"tests/{m}.py {name}.__init__: {diff}"


def test_a_parameter_the_emulation_lacks_is_seen():
    """The comparison itself: a parameter added to the real op only, another default, another name, another order of the
    positional parameters and a missing keyword-only argument are each reported; another order of the keyword-only ones is not."""
    def real(a, b, c=1, *, k=None, j=2):
        pass

    def same(a, b, c=1, *, j=2, k=None):
        pass

    def lacks(a, b, c=1, *, k=None):
        pass

    def lacks_positional(a, b, *, k=None, j=2):
        pass

    def renamed(a, bb, c=1, *, k=None, j=2):
        pass

    def default(a, b, c=2, *, k=None, j=2):
        pass

    def swapped(b, a, c=1, *, k=None, j=2):
        pass

    def kw_default(a, b, c=1, *, k=None, j=3):
        pass

    assert signature_difference(same, real) is None
    for emu in (lacks, lacks_positional, renamed, default, swapped, kw_default):
        assert signature_difference(emu, real) is not None, emu.__name__
