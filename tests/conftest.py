import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (gfx950) GPU and the built native extension")
    config.addinivalue_line("markers", "slow: long-running")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this environment")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


def pytest_sessionfinish(session, exitstatus):
    """Collect the steppers / executors / models of the tests (they reference each other) while the runtime is fully
    up, so the RCCL communicators, graphs and streams they own are not released during interpreter teardown."""
    import gc
    gc.collect()
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        torch.cuda.synchronize()


NATIVE_OWNERS = ("NativeStepper", "CANNetExecutor", "SplitCapture", "BucketedReducer", "CUDAGraph", "ExternalStream")


def pytest_terminal_summary(terminalreporter):
    """After a session that used the GPU: one line with what still owns native resources once the session's garbage
    is collected (steppers, executors, captured graphs, reducers, owned streams) and the process's thread count.
    Whatever is listed here is released by the interpreter's final garbage collection or not at all."""
    torch = sys.modules.get("torch")
    if torch is None or not torch.cuda.is_initialized():
        return
    import gc
    alive = {}
    for o in gc.get_objects():
        name = type(o).__name__
        if name in NATIVE_OWNERS:
            alive[name] = alive.get(name, 0) + 1
    try:
        threads = len(os.listdir("/proc/self/task"))
    except OSError:
        threads = None
    terminalreporter.write_line(f"native teardown audit: alive after the session {alive or 'none'}, threads {threads}")


@pytest.hookimpl(trylast=True)
def pytest_unconfigure(config):
    """Native stack dump on a fatal signal during process teardown (bindings.cpp); installed here, after pytest's
    faulthandler plugin has restored the handler it replaced.  Unconditional once the extension is loaded: the
    intermittent segmentation fault after a GPU suite whose tests all passed strikes inside the interpreter's final
    garbage collection, with no Python frame left, so only the native frames can name what was being released."""
    ext = sys.modules.get("can_distributed_pytorch_amd.ops._ext")
    if ext is not None and ext._mod is not None and hasattr(ext._mod, "segv_trace"):
        ext._mod.segv_trace()


@pytest.fixture
def dispatch_cfg():
    """Switch kernel-dispatch fields for one test (ops/dispatch.py); the previous config is restored after it.
    ``dispatch_cfg(rring=0)`` — the only way a test selects a non-default variant (no environment variables)."""
    import dataclasses
    from can_distributed_pytorch_amd.ops import dispatch
    prev = dispatch.current()

    def set_(**kw):
        dispatch.apply(dataclasses.replace(dispatch.current(), **kw))
    yield set_
    dispatch.apply(prev)
