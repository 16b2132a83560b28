import sys
from pathlib import Path

import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent
if str(REPO_ROOT) not in sys.path:
    sys.path.insert(0, str(REPO_ROOT))


@pytest.fixture
def short_tmp_path():
    """A per-test directory with a SHORT absolute path. The job bridge is a
    Unix-domain socket inside the job's work dir, and sockaddr_un.sun_path
    holds at most 107 bytes; pytest's tmp_path sits under $TMPDIR and the
    user name, which can use that up before the socket name is appended."""
    import shutil
    import tempfile

    d = Path(tempfile.mkdtemp(prefix="hy-", dir="/tmp"))
    yield d
    shutil.rmtree(d, ignore_errors=True)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: requires an MI355X GPU (run via gpurun)")


def pytest_collection_modifyitems(config, items):
    import torch

    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
