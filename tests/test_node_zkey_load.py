"""loadKey and groth16GenProof of the Node.js drop-in (wasmsnark_amd/js) on a snarkjs .zkey, bytes and path: the key goes straight into
a resident handle that carries .vk (wsnark_pkey_load_zkey*).  The files come from the Python side: a model .zkey at 2^4
(tests/zkey_common.py writes it from a synthetic circuit's toxic waste), the witness in both forms, the verification key of the closed
form and the closed form of the proof for fixed r and s (tests/node_zkey_load_check.js).  CPU: the addon's test-only build bound to
the thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import zkey_common as zk
from conftest import ROOT
from wasmsnark_amd import formats, synth

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_domain):
    circ, S, parts, (want_pkey, want_vk) = zk.model(bn, log_domain, "rows")
    wit = synth.witness_bin(circ)
    r, s = bytes([3]) * 32, bytes([5]) * 32
    files = {"model.zkey": zk.zkey_bytes(parts, order=zk.SNARKJS_ORDER), "pkey.bin": want_pkey, "witness.bin": wit,
             "witness.wtns": formats.witness_bin_to_wtns(wit)}
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "vk.json"), "w") as f:
        json.dump(want_vk, f)
    recs = zk.circuit_records(circ)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"nVars": circ.n_vars, "nPublic": circ.n_public, "domain": circ.domain,
                   "records": [sum(x[0] == 0 for x in recs), sum(x[0] == 1 for x in recs)],
                   "r": r.hex(), "s": s.hex(), "proof": synth.expected_proof(circ, S, r, s, bn.mul_base),
                   "public": synth.public_signals(circ)}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_zkey_load_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_zkey_load_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_ZKEY_LOAD_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_zkey_load_on_the_device(tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_ZKEY_LOAD_OK" in out.stdout, out.stdout + out.stderr
