"""Loader of the in-tree native extension (``_C``, built by build_native.py).

No silent fallback: on a machine with a GPU, a missing or stale extension is
an error (``require()`` raises), so GPU tests can never pass on an eager
PyTorch path by accident.
"""
from __future__ import annotations

import importlib
import os

import torch  # noqa: F401  — must be loaded first: _C resolves libamdhip64/librccl to torch's copies

_mod = None
_err = None


def load(build_if_missing: bool = False):
    global _mod, _err
    if _mod is not None:
        return _mod
    name = "_C_asan" if os.environ.get("CANNET_ASAN", "0") == "1" else "_C"   # host-ASan build (build_native --asan)
    try:
        _mod = importlib.import_module("can_distributed_pytorch_amd." + name)
    except ImportError as e:  # pragma: no cover - depends on build state
        _err = e
        if build_if_missing or os.environ.get("CANNET_AUTOBUILD", "0") == "1":
            from .. import build_native
            build_native.build()
            _mod = importlib.import_module("can_distributed_pytorch_amd._C")
            _err = None
    if _mod is not None and os.environ.get("CANNET_SEGV_TRACE", "0") == "1" and hasattr(_mod, "segv_trace"):
        _mod.segv_trace()       # diagnostics: native stack on a fatal signal (bindings.cpp)
    return _mod


def available() -> bool:
    return load() is not None


_checked = False


VARIANT_MARKER = "VARIANT_BUILD_OK"     # written by the A/B variant-build scripts into the variant's package dir


def variant_allowed() -> bool:
    """A/B variant builds (extra hipcc defines, scripts/*/ab_variant_build.sh) load only where the caller opted in:
    ``CANNET_ALLOW_VARIANT_BUILD=1`` or the marker file the variant scripts put next to the variant's package."""
    if os.environ.get("CANNET_ALLOW_VARIANT_BUILD", "0") == "1":
        return True
    return os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), VARIANT_MARKER))


def check_build_flags(m) -> None:
    """Refuse a binary built with extra compile-time flags (an A/B variant left in the production tree) unless the
    caller opted in (variant_allowed)."""
    flags = m.build_flags() if hasattr(m, "build_flags") else ""
    if flags.strip() and not variant_allowed():
        raise RuntimeError(
            f"native extension {m.__file__} is an A/B variant build (extra hipcc flags {flags!r}), not the production "
            f"build; rebuild without CANNET_EXTRA_HIPFLAGS, or set CANNET_ALLOW_VARIANT_BUILD=1 to time it on purpose")


def check_source_hash(m) -> None:
    """Refuse a binary that was not built from the csrc/ sources in this tree (a stale or foreign _C), and a variant
    build with extra compile flags unless opted in (check_build_flags)."""
    from .. import build_native
    check_build_flags(m)
    files = build_native.source_files()
    if not files:                      # installed without sources: nothing to compare against
        return
    want = build_native.source_hash(files)
    got = m.src_hash()
    if got != want:
        raise RuntimeError(
            f"stale native extension: {m.__file__} was built from csrc/ sources with sha256 {got[:16]}..., the tree's "
            f"sources hash to {want[:16]}...; rebuild with `python -m can_distributed_pytorch_amd.build_native`")


def require():
    global _checked
    m = load()
    if m is None:
        raise RuntimeError(
            "can_distributed_pytorch_amd native extension (_C) is not built: run "
            "`python -m can_distributed_pytorch_amd.build_native` (hipcc --offload-arch=gfx950). "
            f"Import error: {_err}")
    if not _checked:
        check_source_hash(m)
        from . import dispatch
        dispatch.apply(dispatch.current())    # the validated $CANNET_DISPATCH config, pushed once
        _checked = True
    return m


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_launch_override = None      # raw stream the native launches go to instead of the current one (launch_on)


class launch_on:
    """``with launch_on(ptr):`` native launches (every ``stream_ptr`` query) go to raw stream ``ptr``.  Unlike
    ``torch.cuda.stream`` it leaves torch's current stream alone (no torch ops may run inside: their allocations
    would be ordered on the current stream) and costs no stream-object churn; the executor issues its
    weight-gradient launches this way."""
    __slots__ = ("ptr", "prev")

    def __init__(self, ptr: int):
        self.ptr = ptr

    def __enter__(self):
        global _launch_override
        self.prev, _launch_override = _launch_override, self.ptr
        return self

    def __exit__(self, *exc):
        global _launch_override
        _launch_override = self.prev
        return False


def own_stream(device) -> "torch.cuda.ExternalStream":
    """A dedicated non-blocking HIP stream on ``device`` (bindings ``stream_create``), wrapped for torch.
    torch.cuda.Stream() hands out its pool's 32 streams round-robin, so a long-lived pool stream can alias one
    another owner takes later (a graph capture's stream).

    The stream lives as long as the process, which releases it at exit.  No finalizer hangs on the wrapper:
    torch's CUDA stream type inherits torch.Stream's weak-reference slot, but its own deallocator frees the object
    without clearing the weak references to it.  A ``weakref.finalize`` on the wrapper therefore never ran, and its
    weak reference kept pointing at the freed wrapper until the interpreter's final garbage collection cleared it
    through that freed memory: an intermittent segmentation fault at exit, once enough steppers had come and gone
    for the memory to be reused."""
    C = require()
    dev = torch.device(device)
    with torch.cuda.device(dev):
        ptr = C.stream_create()
    return torch.cuda.ExternalStream(ptr, device=dev)


def stream_ptr(device=None) -> int:
    """Raw hipStream_t of ``device``'s current stream (the thread's ``torch.cuda.stream`` context and a graph capture
    included).  The raw-stream query skips building a torch.cuda.Stream object: ~5 us -> ~1 us per call, and the
    batch-1 step issues ~60 launches (host profile, profiles/r5/host/)."""
    if _launch_override is not None:
        return _launch_override
    if _raw_stream is not None:
        if device is None:
            idx = torch.cuda.current_device()
        elif isinstance(device, int):
            idx = device
        else:
            if not isinstance(device, torch.device):
                device = torch.device(device)          # "cuda", "cuda:1"
            idx = device.index if device.index is not None else torch.cuda.current_device()
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream
