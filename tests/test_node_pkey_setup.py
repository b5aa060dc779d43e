"""newKey and groupNtt of the Node.js drop-in (wasmsnark_amd/js) against files written by the Python side: powers of tau from known
toxic waste, a circuit's record streams, the closed form of its key under delta = gamma = 1 and after one contribution, and a
transform's expected outputs from the logarithms (tests/node_pkey_setup_check.js).  CPU: the addon's test-only build bound to the
thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import pkey_setup_common as ps
from bn128_ref import le
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_domain):
    from wasmsnark_amd import synth
    circ, S, powers, blobs, (want, (ic, gamma2)) = ps.setup_inputs(bn, log_domain, "columns")
    files = {name + ".bin": powers[name] for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")}
    files.update({name + ".bin": blobs[name] for name in ("polsA", "polsB", "polsC")})
    files["want.bin"] = synth.sections_to_pkey(want)
    files["want_ic.bin"] = b"".join(ic)
    files["want_contributed.bin"] = synth.sections_to_pkey(synth.build_sections(circ, S, bn.mul_base)[0])
    logs = ps.logs_for(log_domain, seed=31)
    for g in (1, 2):
        files["ntt_g%d_in.bin" % g] = ps.points_of_logs(bn, g, logs)
        files["ntt_g%d_fwd.bin" % g] = ps.points_of_logs(bn, g, ps.ntt_logs(logs, False))
        files["ntt_g%d_inv.bin" % g] = ps.points_of_logs(bn, g, ps.ntt_logs(logs, True))
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"domain": circ.domain, "nVars": circ.n_vars, "nPublic": circ.n_public, "delta": le(S.delta).hex(), "badIndex": circ.domain - 3}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_pkey_setup_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_pkey_setup_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 5)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_PKEY_SETUP_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_pkey_setup_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 8)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_PKEY_SETUP_OK" in out.stdout, out.stdout + out.stderr
