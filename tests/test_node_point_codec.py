"""The compressed points and proofs of the Node.js drop-in (wasmsnark_amd/js) against the Python binding: the golden proofs of the t6
key and two planted ones (tests/node_point_codec_check.js).  CPU: the addon's test-only build bound to the thread-emulator library;
-m gpu: the product."""
import json
import os
import shutil
import subprocess

import pytest

import point_codec_common as pc
from conftest import ROOT, load_golden

JS = os.path.join(ROOT, "wasmsnark_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / N-API headers not available")


def _job(bn, path):
    """what Python says, for the script to compare with"""
    import verify_batch_common as vb
    vk, pub = vb._vk("t6")
    proofs = [c["proof"] for c in load_golden("proofs.json")["t6"]]
    job = {"vk": vk, "inputs": pub, "proofs": proofs, "points": {}}
    pts = {g: [p for p in pc.sample_points(g)][:8] for g in (1, 2)}
    for g in (1, 2):
        job["points"][g] = b"".join(pc.key_bytes(g, p) for p in pts[g]).hex()
    for enc in pc.ENCODINGS:
        data, st = bn.compress_proofs(proofs, enc)
        planted = [c for c in pc.planted_proofs(enc, proofs[0]) if c[0] in ("sign of A flipped", "A.x = q")]
        assert len(planted) == 2
        everything = data + b"".join(c[1] for c in planted)
        n = len(everything) // 128
        back, dst = bn.decompress_proofs(everything, enc)
        job[enc] = {"data": data.hex(), "compress_status": st, "planted": b"".join(c[1] for c in planted).hex(),
                    "verify_status": bn.groth16VerifyBatchCompressed(vk, [pub] * n, everything, enc, return_status=True),
                    "decompress_status": dst, "decompressed": back, "points": {}}
        assert job[enc]["verify_status"] == [1] * len(proofs) + [0, 2]
        for g in (1, 2):
            out, pst = bn.compress_points(g, bytes.fromhex(job["points"][g]), enc)
            bad = pc.enc_point(g, pts[g][0], enc) + b"".join(r[1] for r in pc.planted_records(g, enc))
            bad_out, bad_st = bn.decompress_points(g, bad, enc, subgroup=(g == 2))
            assert bad_st[0] == 0 and set(bad_st) >= {0, 1, 2}
            job[enc]["points"][g] = {"data": out.hex(), "status": pst, "bad": bad.hex(), "bad_out": bad_out.hex(), "bad_status": bad_st}
    with open(path, "w") as f:
        json.dump(job, f)
    return 2 * (len(proofs) + 2)


def _run(job, lib=None):
    cmd = ["node", os.path.join(ROOT, "tests", "node_point_codec_check.js"), job] + ([lib] if lib else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900)


@needs_node
def test_node_point_codec_against_emulated_kernels(tmp_path):
    from emul_util import emul_bn128, SO
    n = _job(emul_bn128(), str(tmp_path / "job.json"))
    subprocess.check_call(["make", "-C", JS, "-s", "all", "emul"])
    out = _run(str(tmp_path / "job.json"), SO)
    assert out.returncode == 0 and "NODE_POINT_CODEC_OK %d" % n in out.stdout, out.stdout + out.stderr


@needs_node
@pytest.mark.gpu
def test_node_point_codec_on_gpu(tmp_path):
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    n = _job(wasmsnark_amd.build(device=0), str(tmp_path / "job.json"))
    subprocess.check_call(["make", "-C", JS, "-s"])
    out = _run(str(tmp_path / "job.json"))
    assert out.returncode == 0 and "NODE_POINT_CODEC_OK %d" % n in out.stdout, out.stdout + out.stderr
