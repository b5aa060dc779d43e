"""kzgLoadSrs, kzgCommit, kzgOpen, kzgVerify, polyEval and polyDivide of the Node.js drop-in (wasmsnark_amd/js) against files written
by the Python side: a reference string from a known tau, polynomials, and what tests/kzg_common.py's closed forms say their
commitments, values and proof are; one spoilt proof with the verdict the logarithms give (tests/node_kzg_check.js).  CPU: the
addon's test-only build bound to the thread-emulator library; -m gpu: the product."""
import json
import os
import random
import shutil
import subprocess

import pytest

import kzg_common as kz
from bn128_ref import R
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_n):
    tau_g1, g2_pair, _ = kz.srs_of(bn, log_n)
    n = 1 << log_n
    rnd = random.Random(123)
    polys = [kz.random_poly(rnd, n - 1) for _ in range(3)]
    z, gamma = rnd.randrange(1 << 256), rnd.randrange(R)
    ys, proof = kz.want_open(bn, polys, z, gamma)
    F = [sum(pow(gamma, i, R) * f[k] for i, f in enumerate(polys)) % R for k in range(n - 1)]
    q, _ = kz.py_divide(polys[0], z)
    c_logs, pi_log = [kz.py_eval(f, kz.TAU) for f in polys], kz.py_eval(kz.py_divide(F, z)[0], kz.TAU)
    y_ints = [kz.py_eval(f, z % R) for f in polys]
    assert kz.verdict_of(c_logs, y_ints, z % R, gamma, pi_log) is True and kz.verdict_of(c_logs, y_ints, z % R, gamma, 2 * pi_log) is False
    files = {"tau_g1.bin": tau_g1, "g2_pair.bin": g2_pair, "polys.bin": b"".join(kz.poly_bytes(f) for f in polys),
             "commitments.bin": b"".join(kz.want_commit(bn, f) for f in polys), "ys.bin": b"".join(ys), "proof.bin": proof,
             "spoilt_proof.bin": kz.point_of(bn, 2 * pi_log), "q0.bin": kz.poly_bytes(q)}
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"len": n - 1, "z": kz.le(z).hex(), "gamma": kz.le(gamma).hex(), "spoiltVerdict": False}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_kzg_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


@needs_node
def test_node_kzg_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_KZG_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_kzg_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 8)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_KZG_OK" in out.stdout, out.stdout + out.stderr
