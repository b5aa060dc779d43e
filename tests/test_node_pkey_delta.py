"""contributeKey and verifyContribution of the Node.js drop-in (wasmsnark_amd/js) over a synthetic key, its closed-form re-keyed
twin and tampered variants of that twin (tests/node_pkey_delta_check.js).  CPU: the addon's test-only build bound to the
thread-emulator library; -m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import pkey_check_common as pk
import pkey_delta_common as pd
from conftest import ROOT

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _write_keys(bn, d, log_domain):
    """old.bin / old.wsnark64; want.bin = the closed form under delta * D_FIXED; one file per row of the rejection table, with the
    bits verifyContribution must report bad and the bits it must have run."""
    from wasmsnark_amd import formats, synth
    circ, S, sec = pk.synth_sections(bn, log_domain, seed=23)
    want, _ = pd.closed_form(bn, circ, S, pd.D_FIXED)
    other, _ = pd.closed_form(bn, circ, S, pow(5, 77, pk.R))
    fin_c, fin_h = pk.finite_indices(want, "C"), pk.finite_indices(want, "H")
    cases = {}
    bad = pk.mutable(want)
    bad["pointsC"][64 * fin_c[1]:64 * fin_c[1] + 64] = bytes(want["pointsC"][64 * fin_c[2]:64 * fin_c[2] + 64])
    cases["c_replaced"] = (bad, 4, 31)
    bad = pk.mutable(want)
    j, k = fin_h[1], fin_h[-2]
    bad["pointsH"][64 * j:64 * j + 64], bad["pointsH"][64 * k:64 * k + 64] = bytes(want["pointsH"][64 * k:64 * k + 64]), bytes(want["pointsH"][64 * j:64 * j + 64])
    cases["h_swapped"] = (bad, 8, 31)
    cases["two_scalars"] = (dict(want, pointsH=other["pointsH"]), 8, 31)
    cases["other_delta2"] = (dict(want, delta2=other["delta2"]), 2, 19)
    bad = pk.mutable(want)
    bad["pointsA"][64 * 3 + 40] ^= 1
    cases["a_byte"] = (bad, 1, 31)
    bad = dict(want, polsB=bytearray(want["polsB"]))
    bad["polsB"][8 + 5] ^= 0x10
    cases["polsb_coef"] = (bad, 1, 31)
    off = pk.mutable(want)
    pk.plant(off, "C", fin_c[4], pk.OFF_CURVE)
    files = {"old.bin": sec, "want.bin": want, "off_curve.bin": off}
    files.update({name + ".bin": c[0] for name, c in cases.items()})
    for name, s in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(synth.sections_to_pkey(s))
    formats.write_key_container(sec, os.path.join(d, "old.wsnark64"))
    formats.write_key_container(want, os.path.join(d, "want.wsnark64"))
    expect = {"d": pk.le(pd.D_FIXED).hex(), "cases": {name: {"bad": c[1], "run": c[2]} for name, c in cases.items()}, "off_curve_index": fin_c[4],
              "nC": len(sec["pointsC"]) // 64, "nH": len(sec["pointsH"]) // 64}
    with open(os.path.join(d, "expect.json"), "w") as f:
        json.dump(expect, f)


def _run(d, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_pkey_delta_check.js"), d] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_pkey_delta_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    _write_keys(emul_bn128(), str(tmp_path), 5)
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path), SO)
    assert out.returncode == 0 and "NODE_PKEY_DELTA_OK" in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_pkey_delta_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    _write_keys(wasmsnark_amd.build(device=0), str(tmp_path), 10)
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path))
    assert out.returncode == 0 and "NODE_PKEY_DELTA_OK" in out.stdout, out.stdout + out.stderr
