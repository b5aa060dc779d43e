"""groth16VerifyBatch of the Node.js drop-in (wasmsnark_amd/js) over the reference's 18 verifier cases
(tests/node_verify_batch_check.js).  CPU: the addon's test-only build bound to the thread-emulator library; -m gpu: the product."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _run(lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_verify_batch_check.js")] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_verify_batch_against_emulated_kernels():
    from emul_util import emul_bn128, SO
    emul_bn128()
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(SO)
    assert out.returncode == 0 and "NODE_VERIFY_BATCH_OK 18" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_verify_batch_on_gpu():
    import __graft_entry__
    __graft_entry__.ensure_built()
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run()
    assert out.returncode == 0 and "NODE_VERIFY_BATCH_OK 18" in out.stdout, out.stdout + out.stderr
