import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# torch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's, but torch asks for it by file name): import it before any
# test module loads libmifft.so, so that one HIP runtime serves both.  Loaded the other way round, torch brings a second runtime
# that sees no GPU and the torch-interop tests cannot run (bench.py imports torch first too).
try:
    import torch  # noqa: F401
except Exception:
    pass


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def ctx():
    """HipContext: counterpart of the reference's helpers.CudaContext (test/helpers.py:29-74)."""
    from helpers import HipContext
    return HipContext()
