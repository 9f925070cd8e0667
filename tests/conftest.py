import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cpu_numerics  # noqa: E402

cpu_numerics.apply()      # before anything imports torch: the golden fixtures were captured under the same CPU arithmetic


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def gh_lib_path():
    from guassianhand_amd import _lib
    if _lib.is_stale():
        _lib.build()
    return _lib.LIB_PATH


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")
