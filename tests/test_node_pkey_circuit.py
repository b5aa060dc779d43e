"""checkKeyCircuit of the Node.js drop-in (wasmsnark_amd/js) against files written by the Python side: powers of tau from known toxic
waste, a circuit's record streams, a good key of that circuit after one contribution with its verification key, a key with two points
of A swapped and a verification key with two IC points swapped (tests/node_pkey_circuit_check.js).  CPU: the addon's test-only build
bound to the thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import pkey_check_common as pk
import pkey_circuit_common as pc
import pkey_setup_common as ps
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_domain):
    from wasmsnark_amd import synth
    circ, S, powers, blobs, _ = ps.setup_inputs(bn, log_domain, "columns")
    sec, vk, _ = pc.good_keys(bn, log_domain, "columns")["contributed"]
    files = {name + ".bin": powers[name] for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")}
    files.update({name + ".bin": blobs[name] for name in ("polsA", "polsB", "polsC")})
    files["key.bin"] = synth.sections_to_pkey(sec)
    bad = pk.mutable(sec)
    i, j = pk.finite_indices(sec, "A")[-2:]
    pc._swap(bad["pointsA"], 64, i, j)
    files["tampered_key.bin"] = synth.sections_to_pkey(bad)
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    for name, key in (("vk.json", vk), ("tampered_vk.json", dict(vk, IC=[vk["IC"][1], vk["IC"][0]] + vk["IC"][2:]))):
        with open(os.path.join(d, name), "w") as f:
            json.dump(key, f)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"domain": circ.domain, "nVars": circ.n_vars, "nPublic": circ.n_public}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_pkey_circuit_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_pkey_circuit_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_PKEY_CIRCUIT_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_pkey_circuit_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 8)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_PKEY_CIRCUIT_OK" in out.stdout, out.stdout + out.stderr
