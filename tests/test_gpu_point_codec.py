"""-m gpu: the square roots and the compressed points and proofs (csrc/pointcodec.hip) of the hipcc-built libwsnark.so on the device.
The checks of tests/test_emul_point_codec.py again (tests/point_codec_common.py: every byte against Python integers), then proofs
of the GPU prover itself, compressed and verified."""
import pytest

import point_codec_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__
    __graft_entry__.ensure_built()
    import wasmsnark_amd
    b = wasmsnark_amd.build(device=0)
    assert b.lib.path.endswith("wasmsnark_amd/libwsnark.so")
    return b


def _dev(data):
    import torch
    t = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


@pytest.mark.parametrize("impl", [0, 2])
def test_fq_roots(bn, impl):
    pc.check_fq_roots(bn, impl)


@pytest.mark.parametrize("impl", [0, 2])
def test_fq2_roots(bn, impl):
    pc.check_fq2_roots(bn, impl)


def test_fr_has_no_root(bn):
    pc.check_fr_has_no_root(bn)


def test_literal_vectors(bn):
    pc.check_literal_vectors(bn)


@pytest.mark.parametrize("g", [1, 2])
def test_codec_against_python_integers(bn, g):
    pc.check_codec(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_planted_bad_encodings(bn, g):
    pc.check_planted_points(bn, g)


@pytest.mark.parametrize("g", [1, 2])
def test_more_than_one_chunk(bn, tune, g):
    pc.check_chunked_stream(bn, tune, g)


def test_proof_codec(bn):
    pc.check_proof_codec(bn)


def test_planted_proofs_alone_in_a_batch_and_through_device_pointers(bn):
    pc.check_planted_proofs(bn, _dev)


def test_reference_verifier_vectors_compressed(bn):
    pc.check_golden_verify_compressed(bn)
    pc.check_golden_verify_compressed(bn, "be")


def test_golden_proofs_compressed(bn):
    pc.check_golden_proofs_compressed(bn)


def test_errors_leave_the_outputs_untouched(bn):
    pc.check_errors(bn, bn.lib.path)


def test_proofs_of_the_gpu_prover_compressed(bn):
    """the synthetic key of test_gpu_verify_batch.py::test_proofs_of_the_gpu_prover: sixteen proofs, compressed, all valid; none with
    the wrong public input"""
    from wasmsnark_amd import synth
    circ = synth.make_circuit(12, n_public=2, seed=4)
    S = synth.setup(circ, seed=40)
    pkey, vk = synth.build_key(circ, S, bn.mul_base)
    key = bn.load_key(pkey)
    wit, pub = synth.witness_bin(circ), synth.public_signals(circ)
    proofs = [bn.groth16GenProof(wit, key, r=bytes([i + 1]) * 32, s=bytes([200 - i]) * 32) for i in range(16)]
    key.free()
    wrong = [str((int(pub[0]) + 1) % pc.R)] + pub[1:]
    for enc in pc.ENCODINGS:
        data, st = bn.compress_proofs(proofs, enc)
        assert st == [1] * 16 and data == b"".join(pc.enc_proof(p, enc) for p in proofs)
        assert bn.groth16VerifyBatchCompressed(vk, [pub] * 16, data, enc, return_status=True) == [1] * 16
        assert bn.groth16VerifyBatchCompressed(vk, [wrong] * 16, data, enc) == [False] * 16
        back, st = bn.decompress_proofs(data, enc)
        assert st == [1] * 16 and back == [pc._normal(p) for p in proofs]
