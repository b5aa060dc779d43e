"""checkKey and loadKey(..., {check: true}) of the Node.js drop-in (wasmsnark_amd/js) over a valid and a tampered synthetic key
(tests/node_pkey_check_check.js).  CPU: the addon's test-only build bound to the thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import pkey_check_common as pk
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_keys(bn, d, log_domain):
    from wasmsnark_amd import formats, synth
    circ, S, sec = pk.synth_sections(bn, log_domain, seed=21)
    bad = pk.mutable(sec)
    i = pk.finite_indices(bad, "B2")[4]
    pk.plant(bad, "B2", i, pk.OUTSIDE)
    for name, data in (("good.bin", synth.sections_to_pkey(sec)), ("bad.bin", synth.sections_to_pkey(bad)), ("witness.bin", synth.witness_bin(circ))):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    formats.write_key_container(sec, os.path.join(d, "good.wsnark64"))
    expect = {"bad_index": i, "points": {}, "infinity": {}}
    for s in pk.SECTIONS:
        n = len(sec[pk.SEC_KEY[s]]) // pk.SEC_SIZE[s]
        expect["points"][s], expect["infinity"][s] = n, n - len(pk.finite_indices(sec, s))
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump(expect, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_pkey_check_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_pkey_check_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_keys(emul_bn128(), str(tmp_path), 5)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_PKEY_CHECK_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_pkey_check_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_keys(wasmsnark_amd.build(device=0), str(tmp_path), 10)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_PKEY_CHECK_OK" in out.stdout, out.stdout + out.stderr
