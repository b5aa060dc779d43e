"""mulPoints, contributePowers and checkPowers of the Node.js drop-in (wasmsnark_amd/js) against files written by the Python side: a
transcript from known toxic waste, the closed form of its contribution, a transcript with one replaced power, and per group the
expected products from the logarithms (tests/node_pwtau_check.js).  CPU: the addon's test-only build bound to the thread-emulator
library; -m gpu: the product."""
import json
import os
import random
import shutil
import subprocess

import pytest

import pwtau_common as pw
from bn128_ref import R, le
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_domain, n_mul):
    from wasmsnark_amd import synth
    circ, S, powers = pw.transcript(bn, log_domain)
    want = synth.powers_from_toxic(synth.contributed_toxic(S, pw.T_FIXED, pw.A_FIXED, pw.B_FIXED), circ.domain, bn.mul_base)
    files = {}
    for name in pw.ARRAYS + ("beta_g2",):
        files[name + ".bin"] = powers[name]
        files["want_" + name + ".bin"] = want[name]
    L = pw.logs_of(S, circ.domain)
    L["alpha_tau_g1"][2] = 0xD00D
    assert pw.relations_expected(L) == 8
    files["replaced_alpha_tau_g1.bin"] = pw.ps.points_of_logs(bn, 1, L["alpha_tau_g1"])
    rnd = random.Random(17)
    logs = [rnd.randrange(1, R) for _ in range(n_mul)]
    ks = (pw.planted_scalars()[:12] + [rnd.randrange(1 << 256) for _ in range(n_mul)])[:n_mul]
    files["mul_scalars.bin"] = pw.scalars_bytes(ks)
    for g in (1, 2):
        files["mul_g%d_in.bin" % g] = pw.ps.points_of_logs(bn, g, logs)
        files["mul_g%d_want.bin" % g] = pw.want_products(bn, g, logs, ks)
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"domain": circ.domain, "tau": le(pw.T_FIXED).hex(), "alpha": le(pw.A_FIXED).hex(), "beta": le(pw.B_FIXED).hex(),
                   "badIndex": circ.domain - 3}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_pwtau_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_pwtau_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4, 20)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_PWTAU_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_pwtau_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 8, 300)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_PWTAU_OK" in out.stdout, out.stdout + out.stderr
