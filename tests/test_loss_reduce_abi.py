"""The extension header include/hardnet_mi355x_loss_reduce.h against the binding's table for it, and every argument
check of hn_hardnet_loss_reduce_workspace_bytes / _forward / _backward: return code and message.
No case reaches a launch, so none needs a GPU; with one present the module skips, because the placeholder pointers
must never be able to reach a device (as tests/test_abi_errors.py)."""
import ctypes
import os
import re

import pytest
import torch

from hardnetnas_amd import _native as N

if torch.cuda.is_available():
    pytest.skip("placeholder device pointers: runs on machines without a GPU only", allow_module_level=True)

P = 4096       # a device pointer that is never dereferenced
BIG = 1 << 40  # a workspace size that always suffices
ARG, WORKSPACE = 1, 4  # HN_ERR_ARG, HN_ERR_WORKSPACE
MIN, AVERAGE, RANDOM = 0, 1, 2

FWD = dict(a=P, p=P, idx=P, batch=4, dim=128, reduce=AVERAGE, swap=1, margin=1.0, loss_type=0, loss=P, saved=P,
           saved_bytes=BIG, stream=None)
BWD = dict(a=P, p=P, idx=P, batch=4, dim=128, reduce=AVERAGE, swap=1, margin=1.0, loss_type=0, dloss=P, ga=P, gp=P,
           saved=P, saved_bytes=BIG, stream=None)


def call(name, base, **mods):
    lib = N.load_library()
    rc = getattr(lib, name)(*{**base, **mods}.values())
    return rc, lib.hn_last_error().decode()


def need(reduce, batch):
    n = ctypes.c_size_t()
    assert N.load_library().hn_hardnet_loss_reduce_workspace_bytes(reduce, batch, ctypes.byref(n)) == 0
    return n.value


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _header():
    src = open(os.path.join(ROOT, "include", "hardnet_mi355x_loss_reduce.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_the_enum_is_mirrored():
    assert N.BATCH_REDUCES == {"min": MIN, "average": AVERAGE, "random": RANDOM}
    assert "enum hn_batch_reduce { HN_REDUCE_MIN = 0, HN_REDUCE_AVERAGE = 1, HN_REDUCE_RANDOM = 2 };" in _header()
    main = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    assert '#include "hardnet_mi355x_loss_reduce.h"' in main  # one include gives a C caller the whole ABI


def test_prototypes_agree_with_the_extension_header():
    """Every ``int hn_name(args);`` of the header against the binding's argtypes, name for name (the rule
    test_native_binding.py applies to hardnet_mi355x.h), and the library exports each."""
    decl = {}
    for name, args in re.findall(r"^\s*int\s+(hn_\w+)\s*\(([^)]*)\)\s*;", _header(), re.M):
        params = [" ".join(a.split()) for a in args.split(",")]
        decl[name] = ["pointer" if "*" in a else SCALARS[a.replace("const ", "").split()[0]] for a in params]
    assert sorted(decl) == sorted(N.EXPORTED_LOSS_REDUCE) and len(decl) == 3
    assert not set(decl) & set(N.EXPORTED)
    lib = N.load_library()
    for name, params in decl.items():
        fn = getattr(lib, name)
        got = ["pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else t for t in fn.argtypes]
        assert got == params, name
        assert fn.restype is ctypes.c_int, name


def test_workspace_bytes():
    lib = N.load_library()
    n = ctypes.c_size_t()
    f = lib.hn_hardnet_loss_reduce_workspace_bytes
    # O(B): 'random' is the 'min' layout; 'average' grows linearly (the split partials are bounded by a constant)
    m = ctypes.c_size_t()
    assert lib.hn_hardnet_loss_train_workspace_bytes(4096, ctypes.byref(m)) == 0
    assert need(RANDOM, 4096) == m.value
    assert need(AVERAGE, 65536) <= 4 * 65536 * (2 * 2 * 128 + 64)
    assert need(AVERAGE, 4096) <= 32 << 20 and need(AVERAGE, 1) >= 7 * 256
    for reduce, cap in ((AVERAGE, 65536), (RANDOM, 1 << 22)):
        assert f(reduce, cap, ctypes.byref(n)) == 0 and n.value > 0
        for bad in (0, -1, cap + 1):
            assert f(reduce, bad, ctypes.byref(n)) == ARG and b"batch out of range" in lib.hn_last_error()
        assert f(reduce, 8, None) == ARG
    assert f(MIN, 8, ctypes.byref(n)) == ARG and b"hn_hardnet_loss_train_forward" in lib.hn_last_error()
    for bad in (-1, 3):
        assert f(bad, 8, ctypes.byref(n)) == ARG and b"unknown batch_reduce" in lib.hn_last_error()


CHECKS = [
    ("a NULL", dict(a=None), ARG, "NULL device pointer"),
    ("p NULL", dict(p=None), ARG, "NULL device pointer"),
    ("saved NULL", dict(saved=None), ARG, "NULL device pointer"),
    ("batch 0", dict(batch=0), ARG, "batch out of range"),
    ("average over its cap", dict(batch=65537), ARG, "batch out of range (1 .. 65536 for HN_REDUCE_AVERAGE)"),
    ("random over its cap", dict(reduce=RANDOM, batch=(1 << 22) + 1), ARG, "batch out of range"),
    ("dim", dict(dim=64), ARG, "dim must be 128"),
    ("reduce unknown", dict(reduce=3), ARG, "unknown batch_reduce 3"),
    ("reduce negative", dict(reduce=-1), ARG, "unknown batch_reduce -1"),
    ("reduce min", dict(reduce=MIN), ARG, "hn_hardnet_loss_train_forward"),
    ("loss_type 3", dict(loss_type=3), ARG, "unknown loss_type"),
    ("loss_type -1", dict(loss_type=-1), ARG, "unknown loss_type"),
    ("random without idx", dict(reduce=RANDOM, idx=None), ARG, "HN_REDUCE_RANDOM needs d_idx"),
    ("idx misaligned", dict(reduce=RANDOM, idx=P + 4), ARG, "d_idx must be 8-byte aligned"),
    ("a misaligned", dict(a=P + 4), ARG, "16-byte aligned"),
    ("p misaligned", dict(p=P + 8), ARG, "16-byte aligned"),
    ("saved misaligned", dict(saved=P + 4), ARG, "16-byte aligned"),
    ("saved short", dict(saved_bytes=None), WORKSPACE, "saved workspace too small"),
    ("random saved short", dict(reduce=RANDOM, saved_bytes=None), WORKSPACE, "saved workspace too small"),
]


@pytest.mark.parametrize("entry,base", [("hn_hardnet_loss_reduce_forward", FWD), ("hn_hardnet_loss_reduce_backward", BWD)])
@pytest.mark.parametrize("tag,mods,code,text", CHECKS, ids=[c[0] for c in CHECKS])
def test_shared_argument_checks(entry, base, tag, mods, code, text):
    mods = dict(mods)
    if "saved_bytes" in mods:  # one byte short of the size query's answer
        mods["saved_bytes"] = need(mods.get("reduce", AVERAGE), base["batch"]) - 1
    rc, msg = call(entry, base, **mods)
    assert rc == code and text in msg, (rc, msg)


def test_forward_and_backward_own_checks():
    rc, msg = call("hn_hardnet_loss_reduce_forward", FWD, loss=None)
    assert rc == ARG and "NULL device pointer" in msg
    for k in ("dloss", "ga", "gp"):
        rc, msg = call("hn_hardnet_loss_reduce_backward", BWD, **{k: None})
        assert rc == ARG and "NULL device pointer" in msg, k
    for k in ("ga", "gp"):
        rc, msg = call("hn_hardnet_loss_reduce_backward", BWD, **{k: P + 4})
        assert rc == ARG and "gradient pointers must be 8-byte aligned" in msg, k


def test_average_ignores_idx_in_its_checks():
    """With d_idx NULL the 'average' calls pass every check up to the last one that can fail without a launch."""
    rc, msg = call("hn_hardnet_loss_reduce_forward", FWD, idx=None, loss=None)
    assert rc == ARG and "NULL device pointer" in msg
    rc, msg = call("hn_hardnet_loss_reduce_backward", BWD, idx=None, gp=P + 4)
    assert rc == ARG and "gradient pointers" in msg
