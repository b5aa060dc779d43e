"""checkWitnesses of a loaded circuit and the {circuit} option of groth16GenProofBatch of the Node.js drop-in (wasmsnark_amd/js) against
files written by the Python side: a circuit's three record streams, five witnesses of it back to back (the second and the last break a
constraint of their own), a proving key of the circuit, and what Python integers say about every witness
(tests/node_witness_check_batch.js).  CPU: the addon's test-only build bound to the thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import witness_check_batch_common as wb
import witness_check_common as wc
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")
ROUTE = {"WSNARK_BATCH_MIN": "1", "WSNARK_BATCH_MAX_DOMAIN": "65536"}      # the batch kernels whatever the routing defaults say


def _write_files(bn, d, log_domain):
    from wasmsnark_amd import synth
    circ, blobs, rows3 = wc.synth_case(log_domain)
    wits, wants = wb.batch_case(log_domain, "columns", 5, good={0, 2, 3})
    pkey, vk = synth.build_key(circ, synth.setup(circ, seed=11), bn.mul_base)
    other = wc.synth_case(log_domain + 1)[1]
    files = {name + ".bin": blobs[name] for name in ("polsA", "polsB", "polsC")}
    files.update({"other_" + name + ".bin": other[name] for name in ("polsA", "polsB", "polsC")})
    files.update({"witnesses.bin": b"".join(wc.wbytes(w) for w in wits), "key.bin": pkey})
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"domain": circ.domain, "nVars": circ.n_vars, "nPublic": circ.n_public, "otherNVars": other["n_vars"], "otherDomain": other["domain"],
                   "witnesses": [{"bad": w["bad"], "first_bad": None if w["first_bad"] == wc.NONE else w["first_bad"], "ok": bool(w["ok"]),
                                  "bad_rows": w["bad_rows"], "bad_values": [[str(x) for x in abc] for abc in w["bad_values"]]} for w in wants]}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_witness_check_batch.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, **ROUTE))


@needs_node
def test_node_witness_check_batch_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_WITNESS_CHECK_BATCH_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_witness_check_batch_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 6)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_WITNESS_CHECK_BATCH_OK" in out.stdout, out.stdout + out.stderr
