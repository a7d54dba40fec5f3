"""ctypes binding of libvideosys_amd.so (the C ABI declared in include/videosys_amd.h).

The library is the product: there is NO fallback.  Importing this module on a machine where the shared object has
not been built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C videosys_amd/csrc``) raises.
"""
from __future__ import annotations

import ctypes
import os

from ._opcodes import ENTRY_POINTS, LAB_ENTRY_POINTS

_HERE = os.path.dirname(os.path.abspath(__file__))
# (VSYS_LIB: another build of the same library, e.g. the -DVSYS_LAB flavour the measurement tools load; never a fallback)
LIB_PATH = os.environ.get("VSYS_LIB") or os.path.join(_HERE, "libvideosys_amd.so")

_i64, _f32, _ptr, _int = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int

# name -> argtypes (trailing stream included) of every prototype of include/videosys_amd.h, and of the lab header's pair: built from
# the parameter kinds that csrc/gen/program_gen.py reads off the headers (_opcodes.py), so the binding cannot drift from the C ABI
_KINDS = {"p": _ptr, "l": _i64, "i": _int, "f": _f32, "s": ctypes.c_char_p}
SIGNATURES = {name: [_KINDS[k] for k in args] for name, (args, _) in ENTRY_POINTS.items()}
LAB_SIGNATURES = {name: [_KINDS[k] for k in args] for name, (args, _) in LAB_ENTRY_POINTS.items()}   # -DVSYS_LAB builds only
RESTYPES = {name: _KINDS[ret] for name, (_, ret) in {**ENTRY_POINTS, **LAB_ENTRY_POINTS}.items()}

_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
            "videosys_amd has no CPU/PyTorch fallback for its kernels."
        )
    lib = ctypes.CDLL(LIB_PATH)
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        # (a shipped library from before the current sources — e.g. on a box without hipcc, where build() cannot rebuild it: never run
        #  old kernels against new host code)
        raise RuntimeError(f"{LIB_PATH} is stale: it does not export {missing[:6]}{'...' if len(missing) > 6 else ''} that this version of "
                           "videosys_amd binds; rebuild it on a box with the ROCm compiler (python -c 'import __graft_entry__ as g; g.build()')")
    bound = dict(SIGNATURES)
    if all(hasattr(lib, name) for name in LAB_SIGNATURES):   # -DVSYS_LAB build (include/videosys_amd_lab.h)
        bound.update(LAB_SIGNATURES)
    for name, argtypes in bound.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    _lib = lib
    return lib


class VsysError(RuntimeError):
    pass


def split_args(args, argtypes, keep=None):
    """The arguments of one launch (``argtypes`` = SIGNATURES[name] without the stream) as (tensors, ints, floats): floats in
    declaration order; every other argument as an integer slot, with the tensor a device address came from (ops._p) beside it, or None.
    A ctypes array (a host array the launch reads: copy descriptors) travels as its address and is appended to ``keep``."""
    tensors, ints, floats = [], [], []
    for v, t in zip(args, argtypes):
        if t is _f32:
            floats.append(float(v))
            continue
        tensors.append(getattr(v, "t", None))
        if isinstance(v, ctypes.Array):
            if keep is not None:
                keep.append(v)
            v = ctypes.addressof(v)
        ints.append(0 if v is None else int(v))
    return tensors, ints, floats


# ---- PyTorch custom-op route (csrc/torch_binding.cpp -> libvideosys_torch.so): torch.ops.vsys.launch / torch.ops.vsys.program_run.
# The product path: ops._call and program.Program.run go through the dispatcher whenever the fragment is there (build() compiles
# it); VSYS_TORCH_OPS=0 or a tree without the fragment binds the same extern "C" functions through ctypes instead.
TORCH_LIB_PATH = os.path.join(_HERE, "libvideosys_torch.so")
_torch_ops = False   # False = not looked for yet, None = not available


def torch_ops():
    """``torch.ops.vsys`` with the fragment loaded, or None (ctypes route)."""
    global _torch_ops
    if _torch_ops is False:
        _torch_ops = None
        if os.environ.get("VSYS_TORCH_OPS", "1") != "0" and os.path.exists(TORCH_LIB_PATH) and not os.environ.get("VSYS_LIB"):
            import torch

            load()                                   # libvideosys_amd.so first: the fragment links against it
            try:
                torch.ops.load_library(TORCH_LIB_PATH)
                _torch_ops = torch.ops.vsys
            except OSError as e:                     # (a fragment built against another torch: say so once, use ctypes)
                import warnings

                warnings.warn(f"{TORCH_LIB_PATH} could not be loaded ({e}); the C ABI is bound through ctypes instead")
    return _torch_ops


def check(code: int, what: str):
    if code != 0:
        msg = load().vsys_strerror(code).decode()
        raise VsysError(f"{what}: {msg} (code {code})")
