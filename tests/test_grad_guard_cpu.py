"""The guarded Adam step without a device: FusedAdam's keyword validation, the way the keys travel through Segmentator's optim_dict, the
binding table against the header, and the entry points' argument checks (which return before anything is launched)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_adam(**kw):
    from dct_amd.arch.flat import FlatParams
    from dct_amd.optim import FusedAdam
    params = [torch.nn.Parameter(torch.zeros(7)), torch.nn.Parameter(torch.zeros(3, 2))]
    return FusedAdam(params, lr=1e-3, flat=FlatParams(params), **kw)


@pytest.mark.parametrize("bad", [-1.0, 0, 0.0, float("inf"), float("-inf"), float("nan"), "1.0", True, [1.0]])
def test_max_grad_norm_is_validated(bad):
    with pytest.raises(ValueError, match="dct_amd FusedAdam: max_grad_norm"):
        _flat_adam(max_grad_norm=bad)
    opt = _flat_adam(max_grad_norm=2.0)
    with pytest.raises(ValueError, match="dct_amd FusedAdam: max_grad_norm"):
        opt.set_max_grad_norm(bad)
    assert opt.max_grad_norm == 2.0


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_skip_nonfinite_is_validated(bad):
    with pytest.raises(ValueError, match="dct_amd FusedAdam: skip_nonfinite"):
        _flat_adam(skip_nonfinite=bad)


def test_defaults_are_off_and_switches_are_attributes():
    opt = _flat_adam()
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False and not opt.guarded
    assert opt.last_grad_norm is None and opt.guard_counts() == {"skipped": 0, "clipped": 0}
    assert set(opt.param_groups[0]) >= {"lr", "betas", "eps", "weight_decay"}
    assert "max_grad_norm" not in opt.param_groups[0] and "skip_nonfinite" not in opt.param_groups[0]     # torch's state_dict layout stays
    assert _flat_adam(max_grad_norm=3).max_grad_norm == 3.0 and _flat_adam(max_grad_norm=3).guarded
    assert _flat_adam(skip_nonfinite=True).guarded
    opt = _flat_adam(max_grad_norm=1.5)
    opt.set_max_grad_norm(None)
    assert not opt.guarded
    opt.set_max_grad_norm(0.25)
    assert opt.guarded and opt.max_grad_norm == 0.25


def test_keys_reach_fused_adam_through_segmentator():
    from dct_amd.models import Segmentator
    from dct_amd.optim import FusedAdam
    seg = Segmentator({"name": "unet", "num_classes": 2},
                      {"name": "Adam", "lr": 1e-3, "weight_decay": 1e-4, "max_grad_norm": 0.5, "skip_nonfinite": True},
                      {"name": "StepLR", "step_size": 90, "gamma": 0.1})
    assert isinstance(seg.optimizer, FusedAdam)
    assert seg.optimizer.max_grad_norm == 0.5 and seg.optimizer.skip_nonfinite is True and seg.optimizer.guarded
    with pytest.raises(ValueError, match="dct_amd FusedAdam: max_grad_norm"):
        Segmentator({"name": "unet", "num_classes": 2}, {"name": "Adam", "lr": 1e-3, "max_grad_norm": -2.0},
                    {"name": "StepLR", "step_size": 90, "gamma": 0.1})


def _header_args(name):
    src = open(os.path.join(ROOT, "include", "dct.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w[\w\s]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def _ctype(decl):
    if "*" in decl or decl.startswith("dct_stream"):
        return C.c_void_p
    return {"int64_t": C.c_int64, "size_t": C.c_size_t, "int": C.c_int, "float": C.c_float, "double": C.c_double}[decl.split()[0]]


@pytest.mark.parametrize("name", ["dct_grad_sumsq_workspace_bytes", "dct_grad_sumsq", "dct_adam_flat_dev_guarded"])
def test_binding_table_has_the_headers_signatures(name):
    from dct_amd import _lib
    ret, args = _header_args(name)
    res, argtypes = _lib.SIGNATURES[name]
    assert res is _ctype(ret)
    assert list(argtypes) == [_ctype(a) for a in args]
    assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 101


def test_guarded_entry_point_is_the_unguarded_one_plus_five():
    from dct_amd import _lib
    plain, guarded = _lib.SIGNATURES["dct_adam_flat_dev"][1], _lib.SIGNATURES["dct_adam_flat_dev_guarded"][1]
    assert list(guarded[:len(plain) - 1]) == list(plain[:-1]) and len(guarded) == len(plain) + 5 and guarded[-1] is plain[-1]
    src = open(os.path.join(ROOT, "include", "dct.h")).read()
    rec = re.search(r"typedef struct dct_adam_guard \{(.*?)\} dct_adam_guard;", src, re.S).group(1)
    fields = re.findall(r"\b(double|float|uint32_t|uint64_t)\s+(\w+);", rec)
    assert fields == [("double", "norm"), ("double", "max_norm"), ("float", "coef"), ("uint32_t", "skip"), ("uint64_t", "skipped"),
                      ("uint64_t", "clipped")]
    from dct_amd import hip_ops
    assert hip_ops.GUARD_WORDS * 8 == 8 + 8 + 4 + 4 + 8 + 8


def test_argument_checks_come_before_any_launch():
    """Null pointers, a misaligned gradient buffer and a workspace one byte short are refused with their status codes: the checks sit in
    front of the launches, so made-up addresses never reach the device (there is none here)."""
    from dct_amd import _lib
    lib = _lib.load()
    BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
    n = 3 * 4 * 256 + 2
    nb = lib.dct_grad_sumsq_workspace_bytes(n)
    assert nb == 3 * 8 and lib.dct_grad_sumsq_workspace_bytes(1) == 8 and lib.dct_grad_sumsq_workspace_bytes(1 << 40) == 2048 * 8
    A = 0x10000
    assert lib.dct_grad_sumsq(0, n, A, nb, 0) == BAD_ARG
    assert lib.dct_grad_sumsq(A, n, 0, nb, 0) == BAD_ARG
    assert lib.dct_grad_sumsq(A + 4, n, A, nb, 0) == UNSUPPORTED
    assert lib.dct_grad_sumsq(A, n, A, nb - 1, 0) == WORKSPACE

    def guarded(p=A, g=A, m=A, v=A, state=A, ws=A, nbytes=nb, rec=A):
        return lib.dct_adam_flat_dev_guarded(p, g, m, v, n, state, A, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, ws, nbytes, rec, 1, 1, 0)
    for k in ("p", "g", "m", "v", "state", "ws", "rec"):
        assert guarded(**{k: 0}) == BAD_ARG, k
    assert guarded(g=A + 4) == UNSUPPORTED and guarded(rec=A + 4) == UNSUPPORTED and guarded(ws=A + 2) == UNSUPPORTED
    assert guarded(nbytes=nb - 1) == WORKSPACE
