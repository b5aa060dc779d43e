"""circuitFromRows and loadCircuit({rows}) of the Node.js drop-in (wasmsnark_amd/js) against files written by the Python side: a synth
circuit row by row, the record streams Bn128.circuit_from_rows made of it, a good witness, one with a signal changed, and what the
Python side reports (tests/node_circuit_rows_check.js).  CPU: the addon's test-only build bound to the thread-emulator library;
-m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import circuit_rows_common as cr
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_files(bn, d, log_domain):
    circ, blobs, case, got, (domain, want, report) = cr.e2e_inputs(bn, log_domain, "columns")
    assert [got["polsA"], got["polsB"], got["polsC"]] == want
    rows = cr.pack(case)
    bad = list(circ.witness)
    bad[1 + cr.N_PUBLIC + 2 + 2] = (bad[1 + cr.N_PUBLIC + 2 + 2] + 1) % cr.R      # the output of row 2
    wits = {"good_witness.bin": b"".join(cr.le(v) for v in circ.witness), "bad_witness.bin": b"".join(cr.le(v) for v in bad)}
    rc = bn.load_circuit(rows=rows)
    rep = rc.check_witness(wits["bad_witness.bin"], max_rows=domain)
    rc.free()
    assert rep["bad"] >= 1 and rep["first_bad"] == 2
    files = dict(wits, **{name + ".bin": got[name] for name in ("polsA", "polsB", "polsC")})
    for m in "ABC":
        files.update({m + "_row_ptr.bin": rows[m][0], m + "_col.bin": rows[m][1], m + "_coef.bin": rows[m][2]})
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    n_cons = len(case["cons"])
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump({"nVars": circ.n_vars, "nPublic": circ.n_public, "nConstraints": n_cons, "domain": domain,
                   "domainWithout": max(2, 1 << (n_cons - 1).bit_length()),
                   "report": {"nnz": report["nnz"], "unreduced": report["unreduced"], "zero": report["zero"],
                              "emptySignals": report["empty_signals"], "maxColumn": report["max_column"]},
                   "bad": rep["bad"], "first_bad": rep["first_bad"], "bad_rows": rep["bad_rows"],
                   "bad_values": [[str(x) for x in abc] for abc in rep["bad_values"]]}, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_circuit_rows_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_circuit_rows_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_files(emul_bn128(), str(tmp_path), 4)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_CIRCUIT_ROWS_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_circuit_rows_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_files(wasmsnark_amd.build(device=0), str(tmp_path), 8)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_CIRCUIT_ROWS_OK" in out.stdout, out.stdout + out.stderr
