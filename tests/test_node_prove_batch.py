"""groth16GenProofBatch of the Node.js drop-in (wasmsnark_amd/js; tests/node_prove_batch.js): a batch of 3 equals three groth16GenProof
calls, on the batch kernels (the routing switches set through the environment of the node process) and on the loop over the single
prover.  CPU: the addon's test-only build bound to the thread-emulator library; -m gpu: the product."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")
ROUTES = {"batch": {"WSNARK_BATCH_MIN": "1", "WSNARK_BATCH_MAX_DOMAIN": "65536"}, "loop": {"WSNARK_BATCH_MIN": "4"}}


def _run(route, emul):
    cmd = ["node", os.path.join(ROOT, "tests", "node_prove_batch.js"), "emul" if emul else "product", route]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **ROUTES[route]))


@needs_node
@pytest.mark.parametrize("route", ["batch", "loop"])
def test_node_prove_batch_against_emulated_kernels(route):
    from emul_util import emul_bn128
    emul_bn128()
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(route, True)
    assert out.returncode == 0 and "NODE_PROVE_BATCH_OK %s 3" % route in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["batch", "loop"])
def test_node_prove_batch_on_gpu(route):
    import __graft_entry__
    __graft_entry__.ensure_built()
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(route, False)
    assert out.returncode == 0 and "NODE_PROVE_BATCH_OK %s 3" % route in out.stdout, out.stdout + out.stderr
