"""The Python binding against include/hardnet_mi355x.h, and its call helpers on CPU tensors (no GPU needed):
every prototype of ``_native._PROTOTYPES`` and every mirrored constant is compared with the header's text, and
the helpers every wrapper is written over are pinned where they decide something (the three workspace policies,
output validation, NULL entries of pointer arrays, the alignment copy, the gradient slots)."""
import ctypes
import os
import re

import pytest
import torch

from hardnetnas_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")

SCALARS = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int, "float": ctypes.c_float,
           "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
RESTYPES = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p}


def header():
    src = open(os.path.join(ROOT, "include", "hardnet_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_prototypes():
    """{name: (restype, [ctypes scalar type, or "pointer"])} of every ``int|void|const char* hn_name(args);``."""
    out = {}
    for ret, name, args in re.findall(r"^\s*(int|void|const char\*)\s+(hn_\w+)\s*\(([^)]*)\)\s*;", header(), re.M):
        params = [" ".join(a.split()) for a in args.split(",")]
        if params == ["void"]:
            params = []
        out[name] = (RESTYPES[ret], ["pointer" if "*" in a else SCALARS[a.replace("const ", "").split()[0]]
                                     for a in params])
    return out


def bound_class(t):
    """A ctypes argtype as the header's mapping sees it: "pointer", or the scalar type object itself (c_int32 is
    c_int and c_size_t is c_uint64 here, so objects are compared, never names)."""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return t


def check_prototypes(lib, names):
    """Assert that ``lib``'s argtypes and restype of ``names`` are the header's, name for name."""
    decl = declared_prototypes()
    assert sorted(decl) == sorted(names)
    for name, (restype, params) in decl.items():
        fn = getattr(lib, name)
        assert [bound_class(t) for t in (fn.argtypes or [])] == params, name
        assert fn.restype is restype, name


def test_prototypes_agree_with_the_header():
    decl = declared_prototypes()
    assert len(decl) == 55 and decl["hn_abi_version"][1] == [] and decl["hn_last_error"][1] == []
    check_prototypes(N.load_library(), N.EXPORTED)
    assert N.EXPORTED == list(N._PROTOTYPES)
    lib = N.load_library()
    assert not lib.hn_abi_version.argtypes and not lib.hn_last_error.argtypes


def test_a_table_row_without_a_symbol_raises_at_load(monkeypatch):
    monkeypatch.setitem(N._PROTOTYPES, "hn_no_such_function", (ctypes.c_void_p,))
    monkeypatch.setattr(N, "_lib", None)
    with pytest.raises(AttributeError, match="hn_no_such_function"):
        N.load_library()


def defines():
    return {k: int(v) for k, v in re.findall(r"^#define\s+(HN_\w+)\s+(\d+)\s*$", header(), re.M)}


def enum(name):
    body = re.search(r"enum\s+" + name + r"\s*\{([^}]*)\}", header()).group(1)
    return {k: int(v) for k, v in re.findall(r"(HN_\w+)\s*=\s*(\d+)", body)}


def test_constants_agree_with_the_header():
    d = defines()
    assert N.ABI_VERSION == d["HN_ABI_VERSION"]
    assert N.HN_MAX_LAYERS == d["HN_MAX_LAYERS"]
    assert N.DET_TRAIN_TENSORS == d["HN_DET_TRAIN_TENSORS"]
    kinds = enum("hn_kind")
    assert kinds == {k: getattr(N, k) for k in ("HN_KIND_HARDNET", "HN_KIND_NAS", "HN_KIND_FDL_NASNET",
                                                "HN_KIND_FDL_NASNET01", "HN_KIND_NAS_SUPERNET")}
    assert {"HN_LOSS_" + k.upper(): v for k, v in N.LOSS_TYPES.items()} == enum("hn_loss_type")
    assert {"HN_METRIC_" + k.upper(): v for k, v in N.MATCH_METRICS.items()} == enum("hn_metric")
    # HN_RESIZE_NONE / _CV2_LINEAR / _PIL_BILINEAR: the Python key is the name's first word
    resize = {k[len("HN_RESIZE_"):].split("_")[0].lower(): v for k, v in enum("hn_resize").items()}
    assert resize == N.RESIZE_MODES and len(enum("hn_resize")) == len(N.RESIZE_MODES)


def test_arch_desc_fields_agree_with_the_header():
    body = re.search(r"typedef\s+struct\s+hn_arch_desc\s*\{([^}]*)\}", header()).group(1)
    fields = []
    for ctype, name, dim in re.findall(r"(\w+)\s+(\w+)\s*(?:\[(\w+)\])?\s*;", body):
        t = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[ctype]
        fields.append((name, t * defines()[dim] if dim else t))
    assert len(fields) == 9 and fields == list(N.HnArchDesc._fields_)


# ----------------------------------------------------------------------------------
# the call helpers, on CPU tensors: they compare devices and never touch the GPU
# ----------------------------------------------------------------------------------
def test_out_allocates_accepts_and_rejects():
    t = N._out(None, (3, 128), CPU)
    assert t.shape == (3, 128) and t.dtype == torch.float32 and t.device == CPU and t.is_contiguous()
    assert N._out(None, (2, 4), CPU, dtype=torch.int64).dtype == torch.int64
    assert N._out(t, (3, 128), CPU) is t
    for bad in (torch.empty(3, 64), torch.empty(3, 128, dtype=torch.float64), torch.empty(128, 3).t()):
        with pytest.raises(ValueError, match="out must be"):
            N._out(bad, (3, 128), CPU)
    with pytest.raises(ValueError, match="out must be"):
        N._out(t, (3, 128), torch.device("meta"))
    with pytest.raises(ValueError, match="out_ori must be"):
        N._out(torch.empty(3), (3, 2), CPU, "out_ori")


@pytest.mark.parametrize("need", [15, 16, 4097])
def test_workspace_policies_one_byte_short(need):
    """A supplied buffer of need - 1 bytes under each policy; without one, max(need, 16) fresh bytes."""
    fresh = N._workspace(None, need, CPU)
    assert fresh.dtype == torch.uint8 and fresh.numel() == max(need, 16) and fresh.is_contiguous()
    exact, short = torch.empty(need, dtype=torch.uint8), torch.empty(need - 1, dtype=torch.uint8)
    for policy in ("replace", "raise", "pass"):
        assert N._workspace(exact, need, CPU, too_small=policy) is exact
    got = N._workspace(short, need, CPU)  # replace is the default
    assert got is not short and got.numel() == max(need, 16) and got.dtype == torch.uint8
    with pytest.raises(ValueError, match=f"scratch must be .* at least {need} bytes"):
        N._workspace(short, need, CPU, "scratch", too_small="raise")
    assert N._workspace(short, need, CPU, too_small="pass") is short


@pytest.mark.parametrize("policy", ["replace", "raise", "pass"])
def test_workspace_rejects_wrong_dtype_device_and_layout(policy):
    for bad in (torch.empty(64, dtype=torch.float32), torch.empty(64, 2, dtype=torch.uint8)[:, 0]):
        with pytest.raises(ValueError, match="workspace must be"):
            N._workspace(bad, 16, CPU, too_small=policy)
    with pytest.raises(ValueError, match="saved must be"):
        N._workspace(torch.empty(64, dtype=torch.uint8), 16, torch.device("meta"), "saved", too_small=policy)


def test_ptr_array_keeps_none_as_null():
    a, b = torch.empty(4), torch.empty(2, 3)
    arr = N._ptr_array([a, None, b])
    assert len(arr) == 3 and list(arr) == [a.data_ptr(), None, b.data_ptr()]
    assert len(N._ptr_array([])) == 0


def test_aligned16_copies_only_a_misaligned_view():
    base = torch.arange(3 * 128 + 4, dtype=torch.float32)
    odd = base[1:1 + 3 * 128].view(3, 128).requires_grad_()  # contiguous, 4 bytes past a 16-byte boundary
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    got = N._aligned16(odd)
    assert got.data_ptr() % 16 == 0 and torch.equal(got, odd) and not got.requires_grad
    assert got.untyped_storage().data_ptr() != base.untyped_storage().data_ptr()
    # already aligned: no copy -- the same memory (detach() alone makes it another Python object)
    even = base[4:4 + 3 * 128].view(3, 128)
    assert even.data_ptr() % 16 == 0
    got = N._aligned16(even)
    assert got.data_ptr() == even.data_ptr() and got.shape == even.shape
    assert got.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
    # a strided input is made contiguous first
    assert torch.equal(N._aligned16(torch.arange(12.).view(3, 4).t()), torch.arange(12.).view(3, 4).t())


def test_grad_slots_and_buffers():
    w0 = torch.nn.Parameter(torch.randn(2, 3))
    frozen = torch.nn.Parameter(torch.randn(4), requires_grad=False)
    running = torch.zeros(5)
    w1 = torch.nn.Parameter(torch.randn(3))
    tensors = [w0, frozen, running, w1]
    slots = N._grad_slots(tensors)
    assert slots == [1, 2, 0, 1]
    grads, bufs = N._grad_buffers([w0, w1], slots, tensors)
    assert [g.shape for g in grads] == [w0.shape, w1.shape] and all(g.is_contiguous() for g in grads)
    store = grads[0].untyped_storage().data_ptr()
    assert grads[1].untyped_storage().data_ptr() == store and grads[0].untyped_storage().nbytes() == 4 * (6 + 3)
    assert grads[1].data_ptr() == grads[0].data_ptr() + 4 * 6  # one flat allocation, in parameter order
    assert bufs[0] is grads[0] and bufs[3] is grads[1] and bufs[2] is None
    assert bufs[1].shape == frozen.shape and bufs[1].untyped_storage().data_ptr() != store
    assert bufs[1].data_ptr() != frozen.data_ptr()
