"""ctypes binding of the C ABI in include/hardnet_mi355x.h (libhardnet_mi355x.so).

PyTorch is only plumbing here: it owns device memory (inputs, outputs, workspace via
the caching allocator) and the current HIP stream; all arithmetic of the forward runs
in the library's gfx950 kernels.  ``torch`` is imported before the library is loaded so
that both share the one HIP runtime already mapped by torch (SONAME libamdhip64.so.7).

The module is a prototype table (``_PROTOTYPES``, one row per ABI function), a handful of call
helpers (``_call``, ``_size``, ``_workspace``, ``_out``, ...) and the wrappers over them: a new
entry point is one table row plus the lines that are specific to its wrapper.

There is no fallback: if the library cannot be loaded, every entry point raises.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import threading
import weakref
from typing import Dict, List, Optional

import numpy as np
import torch

from . import arch as A

_LIB_NAME = "libhardnet_mi355x.so"
_lib = None
_lib_lock = threading.Lock()

# mirrors of the header's constants (tests/test_native_binding.py compares them with the header)
HN_KIND_HARDNET = 0
HN_KIND_NAS = 1
HN_KIND_FDL_NASNET = 2
HN_KIND_FDL_NASNET01 = 3
HN_KIND_NAS_SUPERNET = 4  # train mode only (hn_nas_train_*)
HN_MAX_LAYERS = 8
ABI_VERSION = 2   # HN_ABI_VERSION
DET_TRAIN_TENSORS = 40  # HN_DET_TRAIN_TENSORS
LOSS_TYPES = {"triplet_margin": 0, "softmax": 1, "contrastive": 2}  # enum hn_loss_type
BATCH_REDUCES = {"min": 0, "average": 1, "random": 2}  # enum hn_batch_reduce (hardnet_mi355x_loss_reduce.h)
AVERAGE_MAX_BATCH = 65536  # hn_hardnet_loss_reduce_*: the cap of HN_REDUCE_AVERAGE
MATCH_METRICS = {"unit": 0, "l2": 1}  # enum hn_metric
RESIZE_MODES = {"none": 0, "cv2": 1, "pil": 2}  # enum hn_resize


class HnArchDesc(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("op", ctypes.c_int32 * HN_MAX_LAYERS),
        ("c_in", ctypes.c_int32 * HN_MAX_LAYERS),
        ("c_out", ctypes.c_int32 * HN_MAX_LAYERS),
        ("stride", ctypes.c_int32 * HN_MAX_LAYERS),
        ("input_norm_eps", ctypes.c_float),
        ("l2_eps", ctypes.c_float),
        ("bn_eps", ctypes.c_float),
    ]


# ----------------------------------------------------------------------------------
# the prototype table: every ABI function and its argtypes, by subsystem in the header's order
# ----------------------------------------------------------------------------------
P, S, I32, I64, U64, F32 = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64,
                            ctypes.c_float)
SP, PP, D = ctypes.POINTER(S), ctypes.POINTER(P), ctypes.POINTER(HnArchDesc)  # size_t*, pointer array, descriptor

_PROTOTYPES = {
    # model and eval forward
    "hn_param_count": (D, SP),
    "hn_create": (D, P, S, PP),
    "hn_workspace_bytes": (P, I64, SP),
    "hn_forward": (P, P, I64, P, P, S, P),
    # hardest-in-batch distances and loss_HardNet
    "hn_pairdist_workspace_bytes": (I64, SP),
    "hn_pairdist_hardneg": (P, P, I64, I32, I32, P, P, P, S, P),
    "hn_pairdist_rows_workspace_bytes": (I64, I64, SP),
    "hn_pairdist_rows": (P, I64, I64, P, I64, I32, P, P, P, P, S, P),
    "hn_hardnet_loss": (P, P, P, I64, F32, I32, F32, P, P, P),
    "hn_hardnet_loss_train_workspace_bytes": (I64, SP),
    "hn_hardnet_loss_train_forward": (P, P, I64, I32, I32, F32, I32, P, P, S, P),
    "hn_hardnet_loss_backward": (P, P, I64, I32, I32, F32, I32, P, P, P, P, S, P),
    # FDLNet's neighbour-mask loss
    "hn_neimask_loss_workspace_bytes": (I64, SP),
    "hn_neimask_loss_forward": (P, P, P, P, I64, I32, F32, F32, P, P, P, P, S, P),
    "hn_neimask_loss_backward": (P, P, I64, I32, F32, P, P, P, P, S, P),
    # evaluation: FPR95, matching
    "hn_fpr95_workspace_bytes": (I64, SP),
    "hn_fpr95": (P, P, P, I64, I32, P, P, P, S, P),
    "hn_match_workspace_bytes": (I64, I64, SP),
    "hn_match_nn2": (P, I64, P, I64, I32, I32, P, P, P, S, P),
    # uint8 patches
    "hn_preprocess": (P, I64, I32, I32, I32, F32, F32, P, P),
    "hn_workspace_bytes_u8": (P, I64, SP),
    "hn_forward_u8": (P, P, I64, I32, I32, I32, F32, F32, P, P, S, P),
    # keypoints to patches
    "hn_clip_patch": (P, I64, I32, I32, P, P, P, P, I64, P, P),
    "hn_clip_patch_backward": (P, P, I64, I32, I32, P, P, P, P, I64, P, P, P),
    "hn_workspace_bytes_kp": (P, I64, SP),
    "hn_forward_kp": (P, P, I64, I32, I32, P, P, P, P, I64, P, P, S, P),
    # keypoint detector: eval, train, selection
    "hn_det_param_count": (SP,),
    "hn_det_create": (P, S, F32, F32, PP),
    "hn_det_workspace_bytes": (I64, I32, I32, SP),
    "hn_det_forward": (P, P, I64, I32, I32, P, P, P, S, P),
    "hn_det_destroy": (P,),
    "hn_det_train_workspace_bytes": (I64, I32, I32, SP, SP),
    "hn_det_train_forward": (P, I64, I32, I32, PP, F32, F32, F32, P, P, P, S, P, S, P),
    "hn_det_train_backward": (P, P, P, I64, I32, I32, PP, PP, P, S, P, S, P),
    "hn_select_workspace_bytes": (I64, I32, I32, I32, SP),
    "hn_select_keypoints": (P, I64, I32, I32, I32, F32, I32, I32, I32, F32, P, F32, P, P, P, P, P, P, P, P, S, P),
    # homography ground-truth stage
    "hn_warp_score": (P, P, I64, I32, I32, I32, I32, P, P, P),
    "hn_gt_scale_orin": (P, F32, P, P, P, I64, I32, I32, P, P, P),
    "hn_mask_keypoints": (P, I64, I32, I32, I32, P, F32, P, P, P, P, P, P),
    "hn_project_keypoints": (P, I64, P, I64, I32, I32, P, F32, P, I32, P, P, P, P),
    # train mode: stock HardNet, hardnetNAS / supernet / FDLNet
    "hn_hardnet_train_workspace_bytes": (I64, SP, SP),
    "hn_hardnet_train_forward": (P, I64, PP, PP, PP, F32, F32, U64, P, P, S, P, S, P),
    "hn_hardnet_train_backward": (P, I64, PP, PP, P, F32, U64, P, S, P, S, P),
    "hn_hardnet_train_layer_op_workspace_bytes": (I32, I32, I64, SP),
    "hn_hardnet_train_layer_op": (I32, I32, I32, I32, I64, I64, P, P, P, P, P, P, F32, F32, U64, P, S, P),
    "hn_nas_train_tensor_count": (D, SP),
    "hn_nas_train_workspace_bytes": (D, I64, SP, SP),
    "hn_nas_train_forward": (D, P, I64, PP, F32, P, P, P, S, P, S, P),
    "hn_nas_train_backward": (D, P, P, I64, PP, P, PP, P, P, S, P, S, P),
    "hn_nas_train_backward_dx": (D, P, P, I64, PP, P, PP, P, P, P, S, P, S, P),
    # profiling, lifetime, errors
    "hn_set_profiling": (P, ctypes.c_int),
    "hn_stage_times": (P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                       ctypes.POINTER(I64)),
    "hn_destroy": (P,),
    "hn_last_error": (),
    "hn_abi_version": (),
}
# every function returns int (ctypes' default restype) but these
_RESTYPES = {"hn_det_destroy": None, "hn_rfdet_destroy": None, "hn_destroy": None, "hn_last_error": ctypes.c_char_p}
EXPORTED = list(_PROTOTYPES)
# the extension header include/hardnet_mi355x_loss_reduce.h: loss_HardNet's 'average' and 'random' reductions
# (tests/test_loss_reduce_abi.py compares this table with that header)
_LOSS_REDUCE_PROTOTYPES = {
    "hn_hardnet_loss_reduce_workspace_bytes": (I32, I64, SP),
    "hn_hardnet_loss_reduce_forward": (P, P, P, I64, I32, I32, I32, F32, I32, P, P, S, P),
    "hn_hardnet_loss_reduce_backward": (P, P, P, I64, I32, I32, I32, F32, I32, P, P, P, P, S, P),
}
EXPORTED_LOSS_REDUCE = list(_LOSS_REDUCE_PROTOTYPES)
# the extension header include/hardnet_mi355x_rfdet.h: RF-Net's ten-scale detector (tests/test_rfdet.py compares
# this table with that header)
_RFDET_PROTOTYPES = {
    "hn_rfdet_param_count": (SP,),
    "hn_rfdet_create": (P, S, P, F32, F32, F32, PP),
    "hn_rfdet_workspace_bytes": (I64, I32, I32, SP),
    "hn_rfdet_forward": (P, P, I64, I32, I32, P, P, P, P, S, P),
    "hn_rfdet_destroy": (P,),
}
EXPORTED_RFDET = list(_RFDET_PROTOTYPES)
RFDET_PARAM_FLOATS = 21890  # hn_rfdet_param_count


def lib_path() -> str:
    return os.environ.get("HN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", _LIB_NAME)


def load_library():
    """Load (once) and type the C ABI.  Raises if the library is missing, or lacks a function of the table
    (ctypes' AttributeError names the symbol)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f"hardnetnas_amd native library not found at {path}; build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (make -C hardnetnas_amd/csrc)")
        lib = ctypes.CDLL(path)
        for name, argtypes in (list(_PROTOTYPES.items()) + list(_LOSS_REDUCE_PROTOTYPES.items())
                               + list(_RFDET_PROTOTYPES.items())):
            fn = getattr(lib, name)
            fn.argtypes = list(argtypes)
            if name in _RESTYPES:
                fn.restype = _RESTYPES[name]
        if lib.hn_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{path}: ABI version {lib.hn_abi_version()}, expected {ABI_VERSION}; rebuild it")
        _lib = lib
        return lib


# ----------------------------------------------------------------------------------
# call helpers
# ----------------------------------------------------------------------------------
def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().hn_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def _call(dev, name: str, *args):
    """Launch ABI function ``name`` on the current stream of ``dev`` (appended as the last argument) with ``dev``
    the current device, and check its status.  A tensor argument is passed as its data pointer, None as NULL,
    anything else as it is.  Nothing here synchronises: the call stays capturable."""
    fn = getattr(_lib or load_library(), name)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _check(fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], stream), name)


def _size(name: str, *args, n: int = 1):
    """The ``n`` trailing size_t outputs of a ``*_workspace_bytes`` / ``*_count`` function: an int, or a tuple
    (saved, scratch) for n == 2."""
    outs = [ctypes.c_size_t() for _ in range(n)]
    _check(getattr(_lib or load_library(), name)(*args, *outs), name)
    return outs[0].value if n == 1 else tuple(o.value for o in outs)


def _buf(t: torch.Tensor):
    """A uint8 workspace as the (pointer, byte count) pair of arguments the C ABI takes."""
    return t, t.numel()


def _ptr_array(ts):
    """The host array of device pointers of ``ts`` (a None entry is NULL)."""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _workspace(ws, need: int, dev, what: str = "workspace", too_small: str = "replace"):
    """A uint8 buffer for a call that needs ``need`` bytes: a fresh one of max(need, 16) bytes without ``ws``, else
    ``ws`` once its dtype, device and contiguity are checked.  A supplied buffer below ``need`` is, by
    ``too_small``: "replace" -- silently replaced by a fresh one; "raise" -- a ValueError naming the byte count;
    "pass" -- handed on as it is (the C ABI answers HN_ERR_WORKSPACE)."""
    if ws is not None:
        if ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous():
            raise ValueError(f"{what} must be a contiguous uint8 tensor on {dev}")
        if ws.numel() >= need or too_small == "pass":
            return ws
        if too_small == "raise":
            raise ValueError(f"{what} must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    return torch.empty(max(need, 16), device=dev, dtype=torch.uint8)


def _out(t, shape, dev, what: str = "out", dtype=torch.float32):
    """The destination of an output: a fresh tensor without ``t``, else ``t`` once its shape, dtype, device and
    contiguity are checked."""
    if t is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} {list(shape)} tensor on {dev}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t


def _aligned16(x: torch.Tensor) -> torch.Tensor:
    """A contiguous, detached x whose rows the C ABI can take (16-byte aligned: a contiguous view at an odd
    storage offset is copied)."""
    x = x.detach().contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _grad_slots(tensors):
    """Per tensor of a train ABI's table: 1 = a parameter whose gradient is returned, 2 = a frozen parameter (the
    kernels still write its gradient: it gets a throwaway buffer), 0 = a buffer (running statistics)."""
    return [1 if t.requires_grad else 2 if isinstance(t, torch.nn.Parameter) else 0 for t in tensors]


def _grad_buffers(params, slots, tensors):
    """(grads, bufs) of a train backward: ``grads`` are the gradients of ``params`` (the slot-1 tensors in order),
    one allocation handed out as contiguous views of the parameters' shapes (the supernet has ~2,000; autograd
    stores them as .grad without a copy); ``bufs`` is parallel to ``tensors``: those views, a throwaway buffer per
    frozen parameter and None per running statistic."""
    flat = torch.empty(sum(p.numel() for p in params), device=tensors[0].device, dtype=torch.float32)
    grads = [g.view(p.shape) for g, p in zip(flat.split([p.numel() for p in params]), params)]
    it = iter(grads)
    return grads, [next(it) if k == 1 else torch.empty_like(t) if k == 2 else None for k, t in zip(slots, tensors)]


# ----------------------------------------------------------------------------------
# descriptors and parameter blobs
# ----------------------------------------------------------------------------------
def hardnet_desc(input_norm_eps: float = 1e-7, l2_eps: float = 1e-10) -> HnArchDesc:
    return HnArchDesc(kind=HN_KIND_HARDNET, input_norm_eps=input_norm_eps, l2_eps=l2_eps, bn_eps=1e-5)


def nas_desc(ops: List[str], layers=None, input_norm_eps: float = -1.0,
             l2_eps: float = 0.0) -> HnArchDesc:
    layers = layers or A.SEARCH_SPACE2
    d = HnArchDesc(kind=HN_KIND_NAS, n_layers=len(ops), input_norm_eps=input_norm_eps, l2_eps=l2_eps, bn_eps=1e-5)
    for i, (op, (ci, co, s)) in enumerate(zip(ops, layers)):
        d.op[i] = A.CANDIDATE_BLOCKS.index(op)
        d.c_in[i], d.c_out[i], d.stride[i] = ci, co, s
    return d


def fdl_desc(variant: str = "NASNet", input_norm_eps: float = A.FDL_INPUT_NORM_EPS) -> HnArchDesc:
    """FDLNet HardNetNeiMask (latency/NASNet{,_0.1}/model/des.py): the fixed front is implied
    by the kind; the three IRFBlocks are described like NAS layers."""
    d = nas_desc(A.FDL_OPS, A.FDL_LAYERS, input_norm_eps=input_norm_eps, l2_eps=0.0)
    d.kind = HN_KIND_FDL_NASNET if variant == "NASNet" else HN_KIND_FDL_NASNET01
    return d


def state_dict_blob(sd: Dict[str, torch.Tensor]) -> np.ndarray:
    """Concatenate every float tensor of a state_dict in state_dict order, skipping
    ``num_batches_tracked``.  This is exactly the order hn_create parses:
      HardNet: features.{0,3,...,19}.weight followed by the BN running_mean/var;
      NAS:     first.conv/bn(w,b,mean,var), per block pw/dw/pwl ConvBNRelu (and
               se4.op.{1,3}.{weight,bias}) or the skip's 1x1 ConvBNRelu, then
               last_stages.conv_k1.weight + last_stages.batchnorm running stats;
      FDL:     features.0.{weight,bias}, the front's BN stats / 1x1 ConvBN(Relu)s, the
               IRFBlocks as for NAS, the head conv weight + BN running stats."""
    parts = [v.detach().to("cpu", torch.float32).contiguous().reshape(-1).numpy()
             for k, v in sd.items() if not k.endswith("num_batches_tracked")]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def desc_for_module(module) -> HnArchDesc:
    from .model import HardNet, HardNetNAS, HardNetNeiMask, RFDes
    if isinstance(module, (HardNet, RFDes)):  # RFDes: HardNet's body (the Dropout holds no state), 1e-8 / no eps
        return hardnet_desc(module.input_norm_eps, module.l2_eps)
    if isinstance(module, HardNetNeiMask):
        return fdl_desc(module.variant, module.input_norm_eps)
    if isinstance(module, HardNetNAS):
        return nas_desc(module.arch_ops, module.layers)
    raise TypeError(type(module))


_OP_IDS = itertools.count(1)
_BY_ID: "weakref.WeakValueDictionary[int, NativeModel]" = weakref.WeakValueDictionary()


class NativeModel:
    """A device model (packed, BN-folded weights) created through hn_create."""

    def __init__(self, desc: HnArchDesc, blob: np.ndarray, device: torch.device):
        self.op_id = next(_OP_IDS)  # the ``handle`` argument of torch.ops.hardnet_mi355x.forward
        _BY_ID[self.op_id] = self
        self.lib = load_library()
        self.device = torch.device(device)
        self.desc = desc
        n = _size("hn_param_count", desc)
        if n != blob.size:
            raise ValueError(f"parameter blob has {blob.size} floats, library expects {n}")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.hn_create(desc, blob.ctypes.data, blob.size, h), "hn_create")
        self._h = h

    @classmethod
    def from_module(cls, module, device) -> "NativeModel":
        return cls(desc_for_module(module), state_dict_blob(module.state_dict()), device)

    def workspace_bytes(self, batch: int) -> int:
        return _size("hn_workspace_bytes", self._h, batch)

    def workspace_bytes_u8(self, batch: int) -> int:
        return _size("hn_workspace_bytes_u8", self._h, batch)

    def workspace_bytes_kp(self, n: int) -> int:
        return _size("hn_workspace_bytes_kp", self._h, n)

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (1, 32, 32):
            raise ValueError(f"expected fp32 [B,1,32,32], got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        b = x.shape[0]
        out = _out(out, (b, 128), self.device)
        workspace = _workspace(workspace, self.workspace_bytes(b), self.device)
        _call(self.device, "hn_forward", self._h, x, b, out, *_buf(workspace))
        return out

    __call__ = forward

    def forward_u8(self, u8: torch.Tensor, resize: str = "cv2", normalize: bool = True,
                   mean: float = 0.443728476019, std: float = 0.20197947209,
                   out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Descriptors straight from uint8 patches ([n,64,64] / [n,1,64,64]; [n,32,32] for
        resize='none'): the loader transforms (hardnet/HardNet.py:333-337, 345-349) fused into the
        forward -- equal to ``forward(preprocess(u8, ...))`` bit for bit."""
        x, b, hw = _u8_patches(u8, resize, self.device)
        out = _out(out, (b, 128), self.device)
        workspace = _workspace(workspace, self.workspace_bytes_u8(b), self.device)
        _call(self.device, "hn_forward_u8", self._h, x, b, hw, RESIZE_MODES[resize], int(normalize), mean, std, out,
              *_buf(workspace))
        return out

    def forward_keypoints(self, images: torch.Tensor, kpts: torch.Tensor, scale: torch.Tensor,
                          ori: Optional[torch.Tensor], ratio: torch.Tensor, out: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Descriptors [N,128] of keypoints (arguments as ``clip_patch``): the patches are clipped into the
        workspace a chunk at a time and never leave it -- equal to ``forward(clip_patch(...))`` bit for bit."""
        im, kp, sc, orr, ra = _keypoint_args(images, kpts, scale, ori, ratio, self.device)
        n = kp.shape[0]
        out = _out(out, (n, 128), self.device)
        workspace = _workspace(workspace, self.workspace_bytes_kp(n), self.device)
        _call(self.device, "hn_forward_kp", self._h, im, im.shape[0], im.shape[2], im.shape[3], kp, sc, orr, ra, n,
              out, *_buf(workspace))
        return out

    def set_profiling(self, on: bool):
        _check(self.lib.hn_set_profiling(self._h, int(on)), "hn_set_profiling")

    def stage_times(self) -> Dict[str, tuple]:
        """{stage: (total_ms, launches)} accumulated since the last call (waits on the
        recorded events; call after the stream has been synchronised)."""
        n = 32
        names = (ctypes.c_char_p * n)()
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        k = self.lib.hn_stage_times(self._h, n, names, ms, cnt)
        if k < 0:
            _check(-k, "hn_stage_times")
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(k)}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.hn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pairdist_hardneg(anchor: torch.Tensor, positive: torch.Tensor, anchor_swap: bool = False):
    """(pos, min_neg) of loss_HardNet's 'min' batch_reduce (hardnet/Losses.py:87-110),
    computed by the fused kernel without materialising the BxB distance matrix."""
    if anchor.shape != positive.shape or anchor.dim() != 2:
        raise ValueError("anchor/positive must be equal [B,D]")
    a = anchor.contiguous().float()
    p = positive.contiguous().float()
    b, d = a.shape
    ws = _workspace(None, _size("hn_pairdist_workspace_bytes", b), a.device)
    pos = torch.empty(b, device=a.device, dtype=torch.float32)
    mn = torch.empty(b, device=a.device, dtype=torch.float32)
    _call(a.device, "hn_pairdist_hardneg", a, p, b, d, int(anchor_swap), pos, mn, *_buf(ws))
    return pos, mn


def pairdist_rows(anchor_rows: torch.Tensor, row0: int, positive: torch.Tensor, col_min: bool = False):
    """Rows [row0, row0 + n) of loss_HardNet's masked distance matrix (hardnet/Losses.py:95-108)
    between this rank's anchors and all positives: (pos, row_min, col_min or None); col_min[j]
    is the masked minimum of column j over these rows only (all-reduce it with MIN)."""
    a = anchor_rows.contiguous().float()
    p = positive.contiguous().float()
    if a.dim() != 2 or p.dim() != 2 or a.shape[1] != p.shape[1] or a.device != p.device:
        raise ValueError("expected [n,D] anchors and [B,D] positives on one device")
    n, d = a.shape
    b = p.shape[0]
    ws = _workspace(None, _size("hn_pairdist_rows_workspace_bytes", n, b), a.device)
    pos = torch.empty(n, device=a.device, dtype=torch.float32)
    rmin = torch.empty(n, device=a.device, dtype=torch.float32)
    cmin = torch.empty(b, device=a.device, dtype=torch.float32) if col_min else None
    _call(a.device, "hn_pairdist_rows", a, n, int(row0), p, b, d, pos, rmin, cmin, *_buf(ws))
    return pos, rmin, cmin


class HardNetLossFunction(torch.autograd.Function):
    """loss_HardNet with batch_reduce 'min' (hardnet/Losses.py:87-154) and its backward on the fused
    kernels of hn_loss.hip: no B x B matrix, the gradient routed to each row's positive and its
    selected hardest negative as autograd routes it through the reference formulation
    (HardNet.py:408-423).  anchor / positive: [B,128] fp32 HIP tensors."""

    @staticmethod
    def forward(ctx, anchor, positive, anchor_swap, margin, loss_type):
        a, p = _aligned16(anchor), _aligned16(positive)
        b = a.shape[0]
        saved = torch.empty(_size("hn_hardnet_loss_train_workspace_bytes", b), device=a.device, dtype=torch.uint8)
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        swap, margin, lt = ctx.args = (bool(anchor_swap), float(margin), LOSS_TYPES[loss_type])
        _call(a.device, "hn_hardnet_loss_train_forward", a, p, b, a.shape[1], int(swap), margin, lt, loss,
              *_buf(saved))
        ctx.save_for_backward(a, p, saved)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable  # the fused backward records no graph (no double backward)
    def backward(ctx, dloss):
        a, p, saved = ctx.saved_tensors
        swap, margin, lt = ctx.args
        ga, gp = torch.empty_like(a), torch.empty_like(p)
        dl = dloss.detach().to(device=a.device, dtype=torch.float32).contiguous().reshape(1)
        _call(a.device, "hn_hardnet_loss_backward", a, p, a.shape[0], a.shape[1], int(swap), margin, lt, dl, ga, gp,
              *_buf(saved))
        return ga, gp, None, None, None


class HardNetLossReduceFunction(torch.autograd.Function):
    """loss_HardNet with batch_reduce 'average' or 'random' (hardnet/Losses.py:124-138) and its backward on the
    kernels of hn_loss_dense.hip / hn_loss.hip: no B x B matrix, bit-identical call to call.
    ``apply(anchor, positive, idx, reduce, anchor_swap, margin, loss_type)``: anchor / positive [B,128] fp32 HIP
    tensors; ``idx`` the [B] int64 negatives of 'random' (any values: the kernel clamps each to [0, B-1]), None for
    'average'."""

    @staticmethod
    def forward(ctx, anchor, positive, idx, reduce, anchor_swap, margin, loss_type):
        if reduce not in ("average", "random"):
            raise ValueError(f"HardNetLossReduceFunction runs 'average' and 'random', not {reduce!r}")
        a, p = _aligned16(anchor), _aligned16(positive)
        b = a.shape[0]
        if reduce == "random":
            if idx is None or idx.numel() != b:
                raise ValueError("'random' needs one index per row")
            idx = idx.detach().to(device=a.device, dtype=torch.int64).contiguous().reshape(b)
        else:
            idx = None
        kind = BATCH_REDUCES[reduce]
        saved = torch.empty(_size("hn_hardnet_loss_reduce_workspace_bytes", kind, b), device=a.device,
                            dtype=torch.uint8)
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        ctx.args = (kind, int(bool(anchor_swap)), float(margin), LOSS_TYPES[loss_type])
        _call(a.device, "hn_hardnet_loss_reduce_forward", a, p, idx, b, a.shape[1], *ctx.args, loss, *_buf(saved))
        ctx.idx = idx
        ctx.save_for_backward(a, p, saved)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable  # the fused backward records no graph (no double backward)
    def backward(ctx, dloss):
        a, p, saved = ctx.saved_tensors
        ga, gp = torch.empty_like(a), torch.empty_like(p)
        dl = dloss.detach().to(device=a.device, dtype=torch.float32).contiguous().reshape(1)
        _call(a.device, "hn_hardnet_loss_reduce_backward", a, p, ctx.idx, a.shape[0], a.shape[1], *ctx.args, dl, ga,
              gp, *_buf(saved))
        return ga, gp, None, None, None, None, None


def hardnet_loss_saved_argmins(saved: torch.Tensor, b: int):
    """(row argmin [b], column argmin [b]) int64 out of the workspace ``HardNetLossFunction`` saves for its
    backward (``loss.grad_fn.saved_tensors[2]``; the layout above hn_loss_train_saved_bytes in hn_loss.hip:
    sq [2b] f32, then rowbest [b] u64 and colbest [b] u64 -- value bits << 32 | argmin --, each block 256-byte
    aligned).  Read-only.  The column block is written only by a forward with anchor_swap."""
    def al(n):
        return (n + 255) // 256 * 256
    o, blk = al(8 * b), al(8 * b)  # (2b floats take 8b bytes)
    keys = saved[o:o + 2 * blk].view(torch.int64)
    return keys[:b] & 0xffffffff, keys[blk // 8:blk // 8 + b] & 0xffffffff


def neimask_loss_forward(anchor, positive, anchor_kp, positive_kp, margin: float = 1.0, C: float = 5.0):
    """``hn_neimask_loss_forward`` on fp32 [N,128] descriptors and int64 [N,4] keypoints of one HIP device.
    Returns (loss [], pos [N], min_neg [N], saved): ``saved`` is the uint8 workspace the backward reads --
    row keys [N] u64 then column keys [N] u64 (value bits << 32 | argmin), each block 256-byte aligned
    (``neimask_saved_argmins``)."""
    a, p, ak, pk = (_aligned16(x) for x in (anchor, positive, anchor_kp, positive_kp))
    b = a.shape[0]
    saved = torch.empty(_size("hn_neimask_loss_workspace_bytes", b), device=a.device, dtype=torch.uint8)
    loss = torch.empty((), device=a.device, dtype=torch.float32)
    pos, mn = (torch.empty(b, device=a.device, dtype=torch.float32) for _ in range(2))
    _call(a.device, "hn_neimask_loss_forward", a, p, ak, pk, b, a.shape[1], float(margin), float(C), loss, pos, mn,
          *_buf(saved))
    return loss, pos, mn, saved


def neimask_saved_argmins(saved: torch.Tensor, n: int):
    """(row argmin [n], column argmin [n]) int64 out of a neighbour-mask loss workspace."""
    blk = (8 * n + 255) // 256 * 256
    keys = saved[:2 * blk].view(torch.int64)
    return keys[:n] & 0xffffffff, keys[blk // 8:blk // 8 + n] & 0xffffffff


class NeiMaskLossFunction(torch.autograd.Function):
    """FDLNet's neighbour-mask descriptor loss (FDLNet-master/latency/NASNet/model/des.py:57-96) and its
    backward on the fused kernels of hn_neimask.hip: no N x N matrix, the gradient routed to each row's positive
    and its selected hardest negative as autograd routes it through the reference formulation.
    anchor / positive: [N,128] fp32, anchor_kp / positive_kp: [N,4] int64 rows (b, y, x, 0), one HIP device."""

    @staticmethod
    def forward(ctx, anchor, positive, anchor_kp, positive_kp, margin, C):
        a, p = _aligned16(anchor), _aligned16(positive)
        loss, _, _, saved = neimask_loss_forward(a, p, anchor_kp, positive_kp, margin, C)
        ctx.margin = float(margin)
        ctx.save_for_backward(a, p, saved)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable  # the fused backward records no graph (no double backward)
    def backward(ctx, dloss):
        a, p, saved = ctx.saved_tensors
        ga, gp = torch.empty_like(a), torch.empty_like(p)
        dl = dloss.detach().to(device=a.device, dtype=torch.float32).contiguous().reshape(1)
        _call(a.device, "hn_neimask_loss_backward", a, p, a.shape[0], a.shape[1], ctx.margin, dl, ga, gp, *_buf(saved))
        return ga, gp, None, None, None, None


def hardnet_loss(pos: torch.Tensor, row_min: torch.Tensor, col_min: Optional[torch.Tensor] = None,
                 margin: float = 1.0, loss_type: str = "triplet_margin", scale: Optional[float] = None):
    """scale * sum of loss_HardNet's per-row margin loss (Losses.py:142-153; scale defaults to
    1/n = torch.mean) with min_neg = min(row_min, col_min): (loss [1], min_neg [n])."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type must be one of {sorted(LOSS_TYPES)}")
    n = pos.shape[0]
    ps, rm = pos.contiguous().float(), row_min.contiguous().float()
    cm = col_min.contiguous().float() if col_min is not None else None
    mn = torch.empty(n, device=ps.device, dtype=torch.float32)
    loss = torch.empty(1, device=ps.device, dtype=torch.float32)
    _call(ps.device, "hn_hardnet_loss", ps, rm, cm, n, float(margin), LOSS_TYPES[loss_type],
          float(1.0 / n if scale is None else scale), mn, loss)
    return loss, mn


def fpr95(out_a: torch.Tensor, out_p: torch.Tensor, labels: torch.Tensor):
    """(fpr95, pair distances) on device: the eval loop of hardnet/HardNet.py:450-472
    (``sqrt(sum((a-p)^2))`` per pair) + ``ErrorRateAt95Recall`` (EvalMetrics.py:6-19)."""
    if out_a.shape != out_p.shape or out_a.dim() != 2 or labels.numel() != out_a.shape[0]:
        raise ValueError("expected [n,D] descriptors and [n] labels")
    a = out_a.contiguous().float()
    p = out_p.contiguous().float()
    lab = labels.to(device=a.device, dtype=torch.int32).contiguous()
    n, d = a.shape
    ws = _workspace(None, _size("hn_fpr95_workspace_bytes", n), a.device)
    dists = torch.empty(n, device=a.device, dtype=torch.float32)
    res = torch.empty(1, device=a.device, dtype=torch.float64)
    _call(a.device, "hn_fpr95", a, p, lab, n, d, dists, res, *_buf(ws))
    return float(res.item()), dists


def match_workspace_bytes(n_query: int, n_db: int) -> int:
    return _size("hn_match_workspace_bytes", n_query, n_db)


def match_nn2(query: torch.Tensor, db: torch.Tensor, metric: str = "unit",
              workspace: Optional[torch.Tensor] = None):
    """Nearest and second-nearest row of ``db`` [M,128] for every row of ``query`` [N,128] (fp32 HIP
    tensors) without the N x M matrix: (dist [N,2] fp32, idx [N,2] int32), dist[:,0] <= dist[:,1]; with
    M == 1 the second place is (+inf, -1).  metric 'unit' is FDLNet's distance_matrix_vector
    (math_utils.py:8-19, unit descriptors), 'l2' HardNet's (hardnet/Losses.py:5-13).  Equal keys are
    ordered by database index (include/hardnet_mi355x.h).  The workspace comes from torch's caching
    allocator unless one of at least match_workspace_bytes(N, M) bytes is passed."""
    if metric not in MATCH_METRICS:
        raise ValueError(f"metric must be one of {sorted(MATCH_METRICS)}")
    if query.dim() != 2 or db.dim() != 2 or query.shape[1] != db.shape[1] or query.device != db.device:
        raise ValueError("expected [N,D] queries and [M,D] database rows on one device")
    if not query.is_cuda or query.dtype != torch.float32 or db.dtype != torch.float32:
        raise ValueError("expected fp32 HIP tensors")
    q, b = _aligned16(query), _aligned16(db)
    n, d = q.shape
    m = b.shape[0]
    workspace = _workspace(workspace, match_workspace_bytes(n, m), q.device)
    dist = torch.empty((n, 2), device=q.device, dtype=torch.float32)
    idx = torch.empty((n, 2), device=q.device, dtype=torch.int32)
    _call(q.device, "hn_match_nn2", q, n, b, m, d, MATCH_METRICS[metric], dist, idx, *_buf(workspace))
    return dist, idx


def _keypoint_args(images, kpts, scale, ori, ratio, device=None):
    """The validated, contiguous (images, kpts, scale, ori or None, ratio) of hn_clip_patch / hn_forward_kp."""
    dev = images.device if device is None else device
    if not images.is_cuda or images.device != dev:
        raise ValueError(f"images must be a HIP tensor on {dev}, got {images.device}")
    if images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 1:
        raise ValueError(f"images must be fp32 [B,1,H,W], got {images.dtype} {tuple(images.shape)}")
    b, _, h, w = images.shape
    if b < 1 or h < 2 or w < 2:
        raise ValueError(f"images must hold at least one image of at least 2x2 pixels, got {tuple(images.shape)}")
    if kpts.dtype != torch.int64 or kpts.dim() != 2 or kpts.shape[1] != 4 or kpts.device != dev:
        raise ValueError(f"kpts must be int64 [N,4] rows (b, y, x, .) on {dev}, got {kpts.dtype} "
                         f"{tuple(kpts.shape)} on {kpts.device}")
    n = kpts.shape[0]
    if scale.dtype != torch.float32 or scale.numel() != n or scale.device != dev:
        raise ValueError(f"scale must be fp32 [{n}] on {dev}, got {scale.dtype} {tuple(scale.shape)} on {scale.device}")
    if ori is not None and (ori.dtype != torch.float32 or tuple(ori.shape) != (n, 2) or ori.device != dev):
        raise ValueError(f"ori must be None or fp32 [{n},2] (cos, sin) on {dev}, got {ori.dtype} "
                         f"{tuple(ori.shape)} on {ori.device}")
    if ratio.dtype != torch.float32 or ratio.numel() != b or ratio.device != dev:
        raise ValueError(f"ratio must be fp32 [{b}] (im_info[:,0]) on {dev}, got {ratio.dtype} "
                         f"{tuple(ratio.shape)} on {ratio.device}")
    return (images.contiguous(), kpts.contiguous(), scale.contiguous().view(-1),
            ori.contiguous() if ori is not None else None, ratio.contiguous().view(-1))


def clip_patch(images: torch.Tensor, kpts: torch.Tensor, scale: torch.Tensor, ori: Optional[torch.Tensor],
               ratio: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Rotated, scaled 32x32 windows around keypoints, FDLNet's clip_patch (utils/image_utils.py:11-158) in one
    kernel: images fp32 [B,1,H,W], kpts int64 [N,4] rows (b, y, x, .), scale fp32 [N], ori fp32 [N,2] (cos, sin)
    or None, ratio fp32 [B] (im_info[:,0]), all on one HIP device -> fp32 [N,1,32,32].  Column 0 of a keypoint
    selects its image and its ratio; the call reads nothing outside ``images`` whatever the keypoint data
    (include/hardnet_mi355x.h)."""
    im, kp, sc, orr, ra = _keypoint_args(images, kpts, scale, ori, ratio)
    n = kp.shape[0]
    out = _out(out, (n, 1, 32, 32), im.device)
    _call(im.device, "hn_clip_patch", im, im.shape[0], im.shape[2], im.shape[3], kp, sc, orr, ra, n, out)
    return out


def clip_patch_backward(dout: torch.Tensor, images: torch.Tensor, kpts: torch.Tensor, scale: torch.Tensor,
                        ori: Optional[torch.Tensor], ratio: torch.Tensor, want_scale: bool = True,
                        want_ori: bool = True, out_scale: Optional[torch.Tensor] = None,
                        out_ori: Optional[torch.Tensor] = None):
    """Gradients of ``clip_patch`` with respect to ``scale`` [N] and ``ori`` [N,2] given the patches' gradient
    ``dout`` fp32 [N,1,32,32], in one kernel (hn_clip_patch_backward): ``(d_scale or None, d_ori or None)``.  The
    corners are detached as in the reference; the images, the ratio and the keypoint rows get no gradient.
    ``want_ori`` without ``ori`` is an error.  ``out_scale`` / ``out_ori`` are optional contiguous destinations.
    A keypoint's gradient is bit-identical call to call, alone or in any batch; the call reads nothing outside
    ``images`` whatever the keypoint data (include/hardnet_mi355x.h)."""
    im, kp, sc, orr, ra = _keypoint_args(images, kpts, scale, ori, ratio)
    n = kp.shape[0]
    if want_ori and orr is None:
        raise ValueError("want_ori needs ori: without rotation there is no orientation gradient")
    if dout.dtype != torch.float32 or dout.numel() != n * 1024 or dout.device != im.device:
        raise ValueError(f"dout must be fp32 [{n},1,32,32] on {im.device}, got {dout.dtype} {tuple(dout.shape)} "
                         f"on {dout.device}")
    dout = dout.contiguous()
    ds = _out(out_scale, (n,), im.device, "out_scale") if want_scale else None
    do = _out(out_ori, (n, 2), im.device, "out_ori") if want_ori else None
    _call(im.device, "hn_clip_patch_backward", dout, im, im.shape[0], im.shape[2], im.shape[3], kp, sc, orr, ra, n,
          ds, do)
    return ds, do


class ClipPatchFunction(torch.autograd.Function):
    """``clip_patch`` with its backward to ``scale`` and ``ori`` (once differentiable; ``images``, ``kpts`` and
    ``ratio`` get no gradient): one kernel forward, one kernel backward, which computes only the outputs that
    ``ctx.needs_input_grad`` names.  Arguments as ``clip_patch``; ``scale`` may have any shape of N elements."""

    @staticmethod
    def forward(ctx, images, kpts, scale, ori, ratio):
        ctx.scale_shape = scale.shape
        flat = scale.reshape(-1)
        ctx.has_ori = ori is not None
        ctx.save_for_backward(images, kpts, flat, ori if ori is not None else flat.new_empty(0), ratio)
        return clip_patch(images, kpts, flat, ori, ratio)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        images, kpts, scale, ori, ratio = ctx.saved_tensors
        want_scale, want_ori = ctx.needs_input_grad[2], ctx.has_ori and ctx.needs_input_grad[3]
        ds = do = None
        if want_scale or want_ori:
            ds, do = clip_patch_backward(dout, images, kpts, scale, ori if ctx.has_ori else None, ratio,
                                         want_scale=want_scale, want_ori=want_ori)
        return None, None, ds.view(ctx.scale_shape) if ds is not None else None, do, None


class NativeDetector:
    """FDLNet's NASNet keypoint detector on the device (hn_det_create): ``blob`` is ``state_dict_blob`` of an
    ``RFDet.state_dict()`` -- features.0.{weight,bias}; per InvertedResidual banch2.0.weight, banch2.1.{weight,
    bias,running_mean,running_var}, banch2.3.weight, banch2.4.{..}, banch2.5.weight, banch2.6.{..};
    conv.{weight,bias}; insnorm.{weight,bias}; conv_ori.{weight,bias}; insnorm_ori.{weight,bias}."""

    def __init__(self, blob: np.ndarray, device, bn_eps: float = 1e-5, in_eps: float = 1e-5):
        self.lib = load_library()
        self.device = torch.device(device)
        n = _size("hn_det_param_count")
        if n != blob.size:
            raise ValueError(f"parameter blob has {blob.size} floats, library expects {n}")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.hn_det_create(blob.ctypes.data, blob.size, bn_eps, in_eps, h), "hn_det_create")
        self._h = h
        self._ws = None  # workspace cache: grows, never shrinks

    def workspace_bytes(self, n_images: int, height: int, width: int) -> int:
        return _size("hn_det_workspace_bytes", n_images, height, width)

    def forward(self, images: torch.Tensor, score: Optional[torch.Tensor] = None, ori: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None):
        """images fp32 [B,1,H,W] -> (score [B,H,W], ori [B,H,W,2]).  The workspace is cached on the object (or
        pass one of at least workspace_bytes(B, H, W) bytes, as under graph capture of several shapes)."""
        if images.device != self.device or images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 1:
            raise ValueError(f"expected fp32 [B,1,H,W] on {self.device}, got {images.dtype} {tuple(images.shape)} "
                             f"on {images.device}")
        x = images.contiguous()
        b, _, h, w = x.shape
        score = _out(score, (b, h, w), self.device, "score")
        ori = _out(ori, (b, h, w, 2), self.device, "ori")
        need = self.workspace_bytes(b, h, w)
        if workspace is None:  # the grow-only cache: replaced when it is too small for this call
            workspace = self._ws = _workspace(self._ws, need, self.device)
        else:  # a short one is the C ABI's HN_ERR_WORKSPACE
            workspace = _workspace(workspace, need, self.device, too_small="pass")
        _call(self.device, "hn_det_forward", self._h, x, b, h, w, score, ori, *_buf(workspace))
        return score, ori

    __call__ = forward

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.hn_det_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeRFDetector:
    """RF-Net's ten-scale detector on the device (hn_rfdet_create, include/hardnet_mi355x_rfdet.h): ``blob`` is
    ``state_dict_blob`` of an ``RFDetSO.state_dict()`` (21,890 floats: per level conv_k, insnorm_k, conv_s*,
    insnorm_s*; then conv_o3 .. conv_o21), ``scale_list`` its ten scales."""

    def __init__(self, blob: np.ndarray, scale_list, device, in_eps: float = 1e-5, score_com_strength: float = 100.0,
                 scale_com_strength: float = 100.0):
        self.lib = load_library()
        self.device = torch.device(device)
        n = _size("hn_rfdet_param_count")
        if n != blob.size:
            raise ValueError(f"parameter blob has {blob.size} floats, library expects {n}")
        scales = np.ascontiguousarray(np.asarray(scale_list, dtype=np.float32).reshape(-1))
        if scales.size != 10:
            raise ValueError(f"scale_list has {scales.size} values, the detector has 10 levels")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.hn_rfdet_create(blob.ctypes.data, blob.size, scales.ctypes.data, in_eps,
                                            score_com_strength, scale_com_strength, h), "hn_rfdet_create")
        self._h = h
        self._ws = None  # workspace cache: grows, never shrinks

    def workspace_bytes(self, n_images: int, height: int, width: int) -> int:
        return _size("hn_rfdet_workspace_bytes", n_images, height, width)

    def forward(self, images: torch.Tensor, score: Optional[torch.Tensor] = None,
                scale: Optional[torch.Tensor] = None, ori: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None):
        """images fp32 [B,1,H,W] -> (score [B,H,W], scale [B,H,W], ori [B,H,W,2]).  The workspace is cached on the
        object (or pass one of at least workspace_bytes(B, H, W) bytes, as under graph capture of several shapes)."""
        if images.device != self.device or images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 1:
            raise ValueError(f"expected fp32 [B,1,H,W] on {self.device}, got {images.dtype} {tuple(images.shape)} "
                             f"on {images.device}")
        x = images.contiguous()
        b, _, h, w = x.shape
        score = _out(score, (b, h, w), self.device, "score")
        scale = _out(scale, (b, h, w), self.device, "scale")
        ori = _out(ori, (b, h, w, 2), self.device, "ori")
        need = self.workspace_bytes(b, h, w)
        if workspace is None:  # the grow-only cache: replaced when it is too small for this call
            workspace = self._ws = _workspace(self._ws, need, self.device)
        else:  # a short one is the C ABI's HN_ERR_WORKSPACE
            workspace = _workspace(workspace, need, self.device, too_small="pass")
        _call(self.device, "hn_rfdet_forward", self._h, x, b, h, w, score, scale, ori, *_buf(workspace))
        return score, scale, ori

    __call__ = forward

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.hn_rfdet_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------------
# the detector in train() (hn_det_train_*)
# ----------------------------------------------------------------------------------
def det_train_workspace_bytes(n_images: int, height: int, width: int):
    """(saved, scratch) bytes of hn_det_train_forward / _backward."""
    return _size("hn_det_train_workspace_bytes", n_images, height, width, n=2)


def det_train_tensors(det):
    """The 40 float state_dict tensors of an ``RFDet`` the train ABI walks, in order (num_batches_tracked left out)."""
    return [v for k, v in det.state_dict(keep_vars=True).items() if not k.endswith("num_batches_tracked")]


def _det_train_check(images, tensors):
    if (not images.is_cuda or images.dtype != torch.float32 or images.dim() != 4 or images.shape[1] != 1
            or not images.is_contiguous()):
        raise ValueError(f"expected contiguous fp32 [B,1,H,W] images on a HIP device, got {images.dtype} "
                         f"{tuple(images.shape)} on {images.device}")
    if len(tensors) != DET_TRAIN_TENSORS:
        raise ValueError(f"the detector has {DET_TRAIN_TENSORS} float state_dict tensors, got {len(tensors)}")
    for i, t in enumerate(tensors):
        if t.device != images.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"tensor {i} must be contiguous fp32 on {images.device}")


def det_train_forward(images, tensors, bn_eps: float, in_eps: float, momentum: float, score=None, ori=None,
                      saved=None, scratch=None):
    """``hn_det_train_forward``: images fp32 [B,1,H,W] -> (score [B,H,W], ori [B,H,W,2], saved).  ``tensors`` are the
    module's 40 float state tensors (det_train_tensors); the running statistics among them are updated in place.
    ``saved`` is what det_train_backward reads; outputs and workspaces may be passed in."""
    _det_train_check(images, tensors)
    dev = images.device
    b, _, h, w = images.shape
    n_sv, n_sc = det_train_workspace_bytes(b, h, w)
    score = _out(score, (b, h, w), dev, "score")
    ori = _out(ori, (b, h, w, 2), dev, "ori")
    saved = _workspace(saved, n_sv, dev, "saved", too_small="raise")
    scratch = _workspace(scratch, n_sc, dev, "scratch", too_small="raise")
    _call(dev, "hn_det_train_forward", images, b, h, w, _ptr_array(tensors), float(bn_eps), float(in_eps),
          float(momentum), score, ori, *_buf(saved), *_buf(scratch))
    return score, ori, saved


def det_train_backward(dscore, dori, images, tensors, grads, saved, scratch=None):
    """``hn_det_train_backward``: the upstream gradients (either may be None: zero) -> ``grads``, a list parallel to
    ``tensors`` with a buffer for every parameter and None for the running statistics."""
    _det_train_check(images, tensors)
    dev = images.device
    b, _, h, w = images.shape
    scratch = _workspace(scratch, det_train_workspace_bytes(b, h, w)[1], dev, "scratch", too_small="raise")
    for t, shp, what in ((dscore, (b, h, w), "dscore"), (dori, (b, h, w, 2), "dori")):
        if t is not None:
            _out(t, shp, dev, what)
    for t, g in zip(tensors, grads):
        if g is not None and (g.shape != t.shape or g.dtype != torch.float32 or g.device != dev
                              or not g.is_contiguous()):
            raise ValueError("every gradient buffer must be a contiguous fp32 tensor of its parameter's shape")
    _call(dev, "hn_det_train_backward", dscore, dori, images, b, h, w, _ptr_array(tensors), _ptr_array(grads),
          *_buf(saved), *_buf(scratch))
    return grads


class DetTrainFunction(torch.autograd.Function):
    """``RFDet.forward`` with the module in train() on the GPU kernels (BatchNorm on the batch's statistics, running
    statistics updated in place) and its backward to every parameter -- what autograd does over the reference module
    in FDLNet's training step.  ``tensors`` is the module's float state in order (det_train_tensors), ``bn`` its
    BatchNorm modules (num_batches_tracked incremented) and ``params`` the tensors among ``tensors`` that require
    grad, in the same order.  Returns (score [B,H,W,1], ori [B,H,W,2]); the images get no gradient.  Each call keeps
    its own "saved" workspace as a tensor saved for backward."""

    @staticmethod
    def forward(ctx, images, tensors, bn, bn_eps, in_eps, momentum, *params):
        images = _aligned16(images)  # a batch cut out of a larger one may start at any float
        score, ori, saved = det_train_forward(images, tensors, bn_eps, in_eps, momentum)
        torch._foreach_add_([m.num_batches_tracked for m in bn], 1)
        ctx.tensors, ctx.slot = tensors, _grad_slots(tensors)
        ctx.set_materialize_grads(False)  # an unused output's gradient stays None: the kernels' NULL path
        ctx.save_for_backward(saved, images, *params)
        return score.unsqueeze(-1), ori

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dscore, dori):
        saved, images, *params = ctx.saved_tensors
        grads, bufs = _grad_buffers(params, ctx.slot, ctx.tensors)
        det_train_backward(_aligned16(dscore).squeeze(-1) if dscore is not None else None,
                           _aligned16(dori) if dori is not None else None, images, ctx.tensors, bufs, saved)
        return (None, None, None, None, None, None, *grads)


def select_workspace_bytes(n_images: int, height: int, width: int, topk: int) -> int:
    return _size("hn_select_workspace_bytes", n_images, height, width, topk)


def select_keypoints(score: torch.Tensor, border: int, nms_thresh: float, nms_ksize: int, topk: int,
                     gauss_ksize: int, gauss_sigma: float, scale_map: Optional[torch.Tensor] = None,
                     scale_value: float = 32.0, ori_map: Optional[torch.Tensor] = None, dense: bool = False,
                     workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """Keypoints of a score map [B,H,W] (fp32, HIP): RFDet.process + the second top-K + nonzero() + gathers
    (hn_select_keypoints, include/hardnet_mi355x.h).  Returns ``kpts`` [B K,4] int64 rows (b, y, x, 0) in raster
    order per image, ``kscore`` (the raw score), ``kscale`` (from ``scale_map`` [B,H,W] or ``scale_value``),
    ``kori`` [B K,2] from ``ori_map`` [B,H,W,2] (or None), and with ``dense`` also ``score_proc`` [B,H,W] and
    ``topk_mask`` [B,H,W] uint8.  Ties at both top-K steps go to the lowest flat index; NaN counts as 0."""
    if not score.is_cuda or score.dtype != torch.float32 or score.dim() != 3:
        raise ValueError(f"score must be a fp32 HIP tensor [B,H,W], got {score.dtype} {tuple(score.shape)}")
    dev = score.device
    s = score.contiguous()
    b, h, w = s.shape
    sm = _gt_map("scale_map", scale_map, (b, h, w), dev)
    om = _gt_map("ori_map", ori_map, (b, h, w, 2), dev)
    workspace = _workspace(workspace, select_workspace_bytes(b, h, w, topk), dev)
    n = b * topk
    out = {"kpts": torch.empty((n, 4), device=dev, dtype=torch.int64),
           "kscore": torch.empty(n, device=dev, dtype=torch.float32),
           "kscale": torch.empty(n, device=dev, dtype=torch.float32),
           "kori": torch.empty((n, 2), device=dev, dtype=torch.float32) if om is not None else None}
    if dense:
        out["score_proc"] = torch.empty((b, h, w), device=dev, dtype=torch.float32)
        out["topk_mask"] = torch.empty((b, h, w), device=dev, dtype=torch.uint8)
    _call(dev, "hn_select_keypoints", s, b, h, w, border, nms_thresh, nms_ksize, topk, gauss_ksize, gauss_sigma, sm,
          scale_value, om, out["kpts"], out["kscore"], out["kscale"], out["kori"], out.get("score_proc"),
          out.get("topk_mask"), *_buf(workspace))
    return out


# ----------------------------------------------------------------------------------
# homography ground-truth stage (hn_gt.hip)
# ----------------------------------------------------------------------------------
def _gt_map(name, t, shape, dev, dtype=torch.float32):
    """``t`` as the contiguous ``dtype`` tensor of ``shape`` on ``dev`` that the C ABI reads (None stays None)."""
    if t is None:
        return None
    if not t.is_cuda or t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a {dtype} HIP tensor {tuple(shape)} on {dev}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _gt_homo(name, h, b, dev):
    if not h.is_cuda or h.device != dev or h.dtype != torch.float32 or h.numel() != 9 * b:
        raise ValueError(f"{name} must be fp32 [{b},3,3] on {dev}, got {h.dtype} {tuple(h.shape)} on {h.device}")
    return h.contiguous().view(b, 9)


def warp_score(score: torch.Tensor, homo: torch.Tensor, border: int = 8, align_corners: bool = False,
               want_warped: bool = True, want_visible: bool = True):
    """gtscore's two warps in one kernel (hn_warp_score): score fp32 [B,H,W] and homo fp32 [B,3,3] on one HIP device
    -> (warped [B,H,W], visible [B,H,W]); the source reads as 0 within ``border`` pixels of an edge."""
    if not score.is_cuda or score.dtype != torch.float32 or score.dim() != 3:
        raise ValueError(f"score must be a fp32 HIP tensor [B,H,W], got {score.dtype} {tuple(score.shape)}")
    dev = score.device
    s = score.contiguous()
    b, h, w = s.shape
    hm = _gt_homo("homo", homo, b, dev)
    warped = torch.empty((b, h, w), device=dev, dtype=torch.float32) if want_warped else None
    visible = torch.empty((b, h, w), device=dev, dtype=torch.float32) if want_visible else None
    _call(dev, "hn_warp_score", s, hm, b, h, w, int(border), int(bool(align_corners)), warped, visible)
    return warped, visible


def gt_scale_orin(scale_map: Optional[torch.Tensor], ori_map: torch.Tensor, homo12: torch.Tensor,
                  homo21: torch.Tensor, scale_value: float = 32.0):
    """Network.gt_scale_orin in one kernel (hn_gt_scale_orin): ori_map fp32 [B,H,W,2], scale_map fp32 [B,H,W] or None
    (then ``scale_value`` everywhere), homographies fp32 [B,3,3] -> (gt_scale [B,H,W], gt_ori [B,H,W,2])."""
    if not ori_map.is_cuda or ori_map.dtype != torch.float32 or ori_map.dim() != 4 or ori_map.shape[3] != 2:
        raise ValueError(f"ori_map must be a fp32 HIP tensor [B,H,W,2], got {ori_map.dtype} {tuple(ori_map.shape)}")
    dev = ori_map.device
    om = ori_map.contiguous()
    b, h, w, _ = om.shape
    sm = _gt_map("scale_map", scale_map, (b, h, w), dev)
    h12, h21 = _gt_homo("homo12", homo12, b, dev), _gt_homo("homo21", homo21, b, dev)
    gt_scale = torch.empty((b, h, w), device=dev, dtype=torch.float32)
    gt_ori = torch.empty((b, h, w, 2), device=dev, dtype=torch.float32)
    _call(dev, "hn_gt_scale_orin", sm, float(scale_value), om, h12, h21, b, h, w, gt_scale, gt_ori)
    return gt_scale, gt_ori


def mask_keypoints(mask: torch.Tensor, topk: int, scale_map: Optional[torch.Tensor] = None, scale_value: float = 32.0,
                   ori_map: Optional[torch.Tensor] = None, want_counts: bool = False):
    """pair's nonzero() and masked_selects (hn_mask_keypoints): mask uint8 [B,H,W] -> (kpts [B K,4] int64 rows
    (b, y, x, 0) in raster order, kscale [B K], kori [B K,2] or None, counts [B] int32 or None).  An image with fewer
    than K set pixels gets rows (b, 0, 0, 0) for the rest; nothing is read back."""
    if not mask.is_cuda or mask.dtype != torch.uint8 or mask.dim() != 3:
        raise ValueError(f"mask must be a uint8 HIP tensor [B,H,W], got {mask.dtype} {tuple(mask.shape)}")
    dev = mask.device
    m = mask.contiguous()
    b, h, w = m.shape
    sm = _gt_map("scale_map", scale_map, (b, h, w), dev)
    om = _gt_map("ori_map", ori_map, (b, h, w, 2), dev)
    n = b * int(topk)
    kpts = torch.empty((max(n, 0), 4), device=dev, dtype=torch.int64)
    kscale = torch.empty(max(n, 0), device=dev, dtype=torch.float32)
    kori = torch.empty((max(n, 0), 2), device=dev, dtype=torch.float32) if om is not None else None
    counts = torch.empty(b, device=dev, dtype=torch.int32) if want_counts else None
    _call(dev, "hn_mask_keypoints", m, b, h, w, int(topk), sm, float(scale_value), om, kpts, kscale, kori, counts)
    return kpts, kscale, kori, counts


def project_keypoints(kpts: torch.Tensor, homo: torch.Tensor, shape, scale_map: Optional[torch.Tensor] = None,
                      scale_value: float = 32.0, ori_map: Optional[torch.Tensor] = None, clamp: bool = True):
    """ptCltoCr (hn_project_keypoints): kpts int64 [N,4] rows (b, y, x, .), homo fp32 [B,3,3], ``shape`` = (B, H, W) of
    the right image's maps -> (kpts_r [N,4] rows (b, y', x', 0), scale_r [N], ori_r [N,2] or None)."""
    if not kpts.is_cuda or kpts.dtype != torch.int64 or kpts.dim() != 2 or kpts.shape[1] != 4:
        raise ValueError(f"kpts must be an int64 HIP tensor [N,4], got {kpts.dtype} {tuple(kpts.shape)}")
    dev = kpts.device
    kp = kpts.contiguous()
    b, h, w = (int(v) for v in shape)
    hm = _gt_homo("homo", homo, b, dev)
    sm = _gt_map("scale_map", scale_map, (b, h, w), dev)
    om = _gt_map("ori_map", ori_map, (b, h, w, 2), dev)
    n = kp.shape[0]
    kpts_r = torch.empty((n, 4), device=dev, dtype=torch.int64)
    scale_r = torch.empty(n, device=dev, dtype=torch.float32)
    ori_r = torch.empty((n, 2), device=dev, dtype=torch.float32) if om is not None else None
    _call(dev, "hn_project_keypoints", kp, n, hm, b, h, w, sm, float(scale_value), om, int(bool(clamp)), kpts_r,
          scale_r, ori_r)
    return kpts_r, scale_r, ori_r


def _u8_patches(u8, resize, dev=None):
    """The validated, contiguous uint8 patches of hn_preprocess / hn_forward_u8 with their count and their side."""
    if resize not in RESIZE_MODES:
        raise ValueError(f"resize must be one of {sorted(RESIZE_MODES)}")
    if u8.dtype != torch.uint8 or not u8.is_cuda or dev not in (None, u8.device):
        raise ValueError("expected a uint8 HIP tensor" + (f" on {dev}" if dev is not None else ""))
    hw = 32 if resize == "none" else 64
    n = u8.shape[0]
    if u8.numel() != n * hw * hw:
        raise ValueError(f"expected {hw}x{hw} patches, got shape {tuple(u8.shape)}")
    return u8.contiguous(), n, hw


def preprocess(u8: torch.Tensor, resize: str = "cv2", normalize: bool = True,
               mean: float = 0.443728476019, std: float = 0.20197947209,
               out: torch.Tensor = None) -> torch.Tensor:
    """uint8 patches [n,64,64] (or [n,1,64,64] / [n,64,64,1]; [n,32,32] for resize='none')
    -> fp32 [n,1,32,32] on device, bit-exact with the reference loaders:
    resize='cv2' + normalize = ``transform`` (hardnet/HardNet.py:345-349, cv2_scale Utils.py:10-11);
    resize='pil', normalize=False = augmented ``transform_test`` (HardNet.py:333-337).
    Defaults for mean/std are the reference's --mean-image/--std-image (HardNet.py:86-89)."""
    x, n, hw = _u8_patches(u8, resize)
    out = _out(out, (n, 1, 32, 32), x.device)
    _call(x.device, "hn_preprocess", x, n, hw, RESIZE_MODES[resize], int(normalize), mean, std, out)
    return out


# ----------------------------------------------------------------------------------
# torch.library registration: hardnet_mi355x::forward(Tensor x, int handle) -> Tensor
# ----------------------------------------------------------------------------------
@torch.library.custom_op("hardnet_mi355x::forward", mutates_args=(), device_types="cuda")
def forward_op(x: torch.Tensor, handle: int) -> torch.Tensor:
    """Eval-mode descriptor forward of the NativeModel whose ``op_id`` is ``handle`` (the
    drop-in for HardNet.forward, hardnet/HardNet.py:312-315, under torch.no_grad -- :454).
    Registered as a custom op with a fake (meta) kernel so that torch.compile traces through
    the module's forward; there is no CPU kernel (the CPU path is the module's torch layers)."""
    nm = _BY_ID.get(int(handle))
    if nm is None:
        raise RuntimeError(f"hardnet_mi355x::forward: no live native model with handle {handle}")
    return nm.forward(x)


@forward_op.register_fake
def _forward_fake(x, handle):
    if x.dim() != 4 or tuple(x.shape[1:]) != (1, 32, 32):
        raise ValueError(f"expected [B,1,32,32], got {tuple(x.shape)}")
    return x.new_empty((x.shape[0], 128))


# ----------------------------------------------------------------------------------
# train-mode stock HardNet (hn_hardnet_train_*): an autograd.Function over the C ABI
# ----------------------------------------------------------------------------------
HARDNET_CONV_IDX = (0, 3, 6, 9, 12, 15, 19)   # features.{i}.weight (HardNet.py:280-301)
HARDNET_BN_IDX = (1, 4, 7, 10, 13, 16, 20)


def train_workspace_bytes(batch: int):
    """(saved, scratch) bytes of hn_hardnet_train_forward / _backward for a batch."""
    return _size("hn_hardnet_train_workspace_bytes", batch, n=2)


class HardNetTrainFunction(torch.autograd.Function):
    """model.train() forward of the stock HardNet on the GPU kernels (BatchNorm batch
    statistics + running-statistics update, Dropout, L2Norm) and its backward to the 7 conv
    weights and the input -- what autograd does over the reference module in the training loop
    (hardnet/HardNet.py:379-441).  ``bn`` is a list of the 7 BatchNorm2d modules (their running
    buffers are updated in place, num_batches_tracked incremented).

    Each call keeps its own "saved" workspace (the BN outputs the backward reads) as a tensor
    saved for backward, so the loop's two forwards (anchors, positives; HardNet.py:392-393) each
    hold theirs until ``loss.backward()``, autograd frees it after the backward (or keeps it for
    ``retain_graph=True``: the backward only reads it), and a second backward without
    ``retain_graph`` raises torch's usual error.  The scratch workspace is transient."""

    @staticmethod
    def forward(ctx, x, drop_p, seed, bn, *weights):
        b = x.shape[0]
        n_sv, n_sc = train_workspace_bytes(b)
        saved = torch.empty(n_sv, device=x.device, dtype=torch.uint8)
        scratch = torch.empty(n_sc, device=x.device, dtype=torch.uint8)
        out = torch.empty((b, 128), device=x.device, dtype=torch.float32)
        ws_w = [w.detach().contiguous() for w in weights]
        _call(x.device, "hn_hardnet_train_forward", x, b, _ptr_array(ws_w), _ptr_array([m.running_mean for m in bn]),
              _ptr_array([m.running_var for m in bn]), float(bn[0].momentum), float(drop_p), int(seed), out,
              *_buf(saved), *_buf(scratch))
        del scratch
        torch._foreach_add_([m.num_batches_tracked for m in bn], 1)  # one launch for the 7 counters
        ctx.drop_p, ctx.seed, ctx.b = float(drop_p), int(seed), b
        ctx.save_for_backward(saved, *ws_w)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, *ws_w = ctx.saved_tensors
        dws = [torch.empty_like(w) for w in ws_w]
        need_x = ctx.needs_input_grad[0]
        din = torch.empty((ctx.b, 1, 32, 32), device=dout.device, dtype=torch.float32) if need_x else None
        scratch = torch.empty(train_workspace_bytes(ctx.b)[1], device=dout.device, dtype=torch.uint8)
        _call(dout.device, "hn_hardnet_train_backward", dout.contiguous(), ctx.b, _ptr_array(ws_w), _ptr_array(dws),
              din, ctx.drop_p, ctx.seed, *_buf(saved), *_buf(scratch))
        return (din, None, None, None, *dws)


TRAIN_OPS = {"input_norm": 0, "conv_fwd": 1, "bn_fwd": 2, "l2_fwd": 3, "l2_bwd": 4, "bn_bwd": 5, "conv_wgrad": 6,
             "conv_dgrad": 7, "input_norm_bwd": 8}  # enum hn_train_op


def train_layer_op_workspace_bytes(batch: int, bits: int = -1, row_segments: int = 0) -> int:
    return _size("hn_hardnet_train_layer_op_workspace_bytes", bits, row_segments, batch)


def train_layer_op(op: str, layer: int, batch: int, x=None, w=None, y=None, aux=(None, None, None), bits: int = -1,
                   row_segments: int = 0, dgrad_chunk: int = 0, momentum: float = 0.1, dropout_p: float = 0.0,
                   seed: int = 0, scratch=None):
    """One layer operation of the HardNet train step on caller-owned CNHW buffers (hn_hardnet_train_layer_op, a test
    and diagnostic entry; the header's table gives each operation's x / w / y / aux).  Nothing is allocated but the
    scratch, when none is given."""
    need = train_layer_op_workspace_bytes(batch, bits, row_segments)
    scratch = _workspace(scratch, need, y.device, "scratch", too_small="raise")
    _call(y.device, "hn_hardnet_train_layer_op", TRAIN_OPS[op], layer, bits, row_segments, dgrad_chunk, batch, x, w, y,
          *aux, momentum, dropout_p, seed, *_buf(scratch))
    return y


# ----------------------------------------------------------------------------------
# train-mode hardnetNAS (hn_nas_train_*): the sampled descriptor and the supernet
# ----------------------------------------------------------------------------------
def supernet_desc(layers=None) -> HnArchDesc:
    """HN_KIND_NAS_SUPERNET: every layer a MixedOperation over all 17 CANDIDATE_BLOCKS
    (model_supernet.py:10-36, 53-68)."""
    layers = layers or A.SEARCH_SPACE2
    d = nas_desc(["skip"] * len(layers), layers)
    d.kind = HN_KIND_NAS_SUPERNET
    return d


def train_tensors(module):
    """The float state_dict tensors the train ABI walks, in order (num_batches_tracked and the
    supernet's thetas left out), as (names, tensors)."""
    kept = [(k, v) for k, v in module.state_dict(keep_vars=True).items()
            if not k.endswith(("num_batches_tracked", ".thetas"))]
    return [k for k, _ in kept], [v for _, v in kept]


def nas_train_workspace_bytes(desc: HnArchDesc, batch: int):
    """(saved, scratch) bytes of hn_nas_train_forward / _backward for a descriptor and a batch."""
    return _size("hn_nas_train_workspace_bytes", desc, batch, n=2)


class NasTrainFunction(torch.autograd.Function):
    """model.train() forward of a hardnetNAS descriptor (``desc`` kind NAS) or of the supernet
    (kind NAS_SUPERNET, with the per-layer soft weights ``soft`` [n_layers, 17]) on the GPU
    kernels, and its backward to every parameter (and to ``soft``, and to ``x`` when it requires grad:
    hn_nas_train_backward_dx) -- what autograd does over the
    reference modules in hardnetNAS/supernet_functions/training_functions_supernet.py:88-103.
    ``tensors`` is the module's float state_dict in order (train_tensors); ``params`` are the ones
    among them that are parameters, in the same order; running buffers are updated in place."""

    @staticmethod
    def forward(ctx, x, soft, desc, tensors, momentum, *params):
        b = x.shape[0]
        nt = _size("hn_nas_train_tensor_count", desc)
        if len(tensors) != nt:
            raise ValueError(f"the module has {len(tensors)} float state_dict tensors, the descriptor walks {nt}")
        if soft is not None:
            n_layers = int(desc.n_layers)
            if tuple(soft.shape) != (n_layers, 17) or soft.device != x.device or soft.dtype != torch.float32:
                raise ValueError(f"soft must be fp32 [{n_layers}, 17] on {x.device}, got {soft.dtype} "
                                 f"{tuple(soft.shape)} on {soft.device}")
        n_sv, n_sc = nas_train_workspace_bytes(desc, b)
        saved = torch.empty(n_sv, device=x.device, dtype=torch.uint8)
        scratch = torch.empty(n_sc, device=x.device, dtype=torch.uint8)
        out = torch.empty((b, 128), device=x.device, dtype=torch.float32)
        soft_c = soft.detach().contiguous() if soft is not None else None
        _call(x.device, "hn_nas_train_forward", desc, x, b, _ptr_array(tensors), float(momentum), soft_c, out,
              *_buf(saved), *_buf(scratch))
        del scratch
        ctx.desc, ctx.tensors, ctx.b, ctx.slot = desc, tensors, b, _grad_slots(tensors)
        ctx.has_soft = soft is not None
        ctx.save_for_backward(saved, x, soft_c if soft_c is not None else x.new_empty(0), *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, x, soft_c, *params = ctx.saved_tensors
        grads, bufs = _grad_buffers(params, ctx.slot, ctx.tensors)
        scratch = torch.empty(nas_train_workspace_bytes(ctx.desc, ctx.b)[1], device=dout.device, dtype=torch.uint8)
        dsoft = torch.empty_like(soft_c) if ctx.has_soft else None
        # the input gradient (conv0's data gradient through input_norm) only when the patches need one
        din = torch.empty((ctx.b, 1, 32, 32), device=dout.device, dtype=torch.float32) \
            if ctx.needs_input_grad[0] else None
        _call(dout.device, "hn_nas_train_backward_dx", ctx.desc, dout.contiguous(), x, ctx.b, _ptr_array(ctx.tensors),
              soft_c if ctx.has_soft else None, _ptr_array(bufs), dsoft, din, *_buf(saved), *_buf(scratch))
        return (din, dsoft, None, None, None, *grads)
