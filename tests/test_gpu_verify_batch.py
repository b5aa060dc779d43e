"""-m gpu: the batch verifier (wsnark_groth16_verify_batch[_dev], csrc/pairing.hip) of the hipcc-built libwsnark.so on the
device.  The checks of tests/test_emul_verify_batch.py again (tests/verify_batch_common.py: every status against the pinned
single-proof host verifier), then what only a device can show: thousands of forged proofs in one call, host- and
device-pointer variants, proofs of the GPU prover itself, and calls from several host threads."""
import ctypes as C
import random
import threading

import pytest

import verify_batch_common as vb

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


def test_fp12_device_against_host(bn):
    vb.check_fp12(bn, n_random=16)


def test_reference_verifier_vectors_in_one_batch_and_alone(bn):
    vb.check_golden_verify(bn)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_proofs_in_one_batch(bn, name):
    vb.check_golden_proofs(bn, name)


def test_malformed_proofs_between_valid_neighbours(bn):
    vb.check_mixed_batches(bn, sizes=(1, 2, 63, 65, 131, 1001))


def test_key_level_outcomes(bn):
    vb.check_key_level(bn, bn.lib.path)


def test_python_argument_errors(bn):
    vb.check_python_argument_errors(bn)


@pytest.mark.parametrize("n_public", [1, 5])
def test_forged_proofs_and_flipped_bits(bn, n_public):
    vb.check_forged(bn, n_public, 96)


def test_plain_exponent_gives_the_same_statuses(bn, tune):
    """The cross-check path (the host verifier's 2790-bit exponent on the device) against the shipped split exponentiation."""
    F = vb.Forger(bn, 2, seed=21)
    ib, pb = F.forge(64)
    tp, want = vb.tamper(pb, range(0, 64, 4), random.Random(2))
    split = vb.batch_status(bn.lib, F.vk_bytes(), 2, ib, tp)
    tune(bn.lib, "VERIFY_PLAIN_EXP", 1)
    assert vb.batch_status(bn.lib, F.vk_bytes(), 2, ib, tp) == split == [want.get(i, 1) for i in range(64)]
    tune(bn.lib, "VERIFY_PLAIN_EXP", 2)         # the hard part by square-and-multiply
    assert vb.batch_status(bn.lib, F.vk_bytes(), 2, ib, tp) == split


def test_mul_base_gives_the_reference_points(bn):
    vb.check_mul_base_against_reference(bn)


@pytest.mark.parametrize("what", ["rows", "alone", "host", "shuffled"])
def test_planted_keys_inputs_and_proofs(bn, what):
    vb.check_planted(bn, what=(what,))


@pytest.mark.parametrize("plain", [1, 2])
def test_planted_with_the_plain_exponents(bn, tune, plain):
    vb.check_planted(bn, what=("shuffled",), plain=plain, tune=tune)


def test_planted_through_device_pointers(bn):
    """Every key's shuffled batch again with inputs and proofs resident on the device (no inputs: a null pointer)."""
    import torch
    ones = 0
    for F, mixed in vb.shuffled_key_batches():
        vkb, n = F.vk_bytes(), len(mixed)
        d_pr = torch.frombuffer(bytearray(b"".join(c["proof"] for c in mixed)), dtype=torch.uint8).cuda()
        d_in = torch.frombuffer(bytearray(b"".join(vb._inputs_bytes(c["x"]) for c in mixed)), dtype=torch.uint8).cuda() if F.n_public else None
        torch.cuda.synchronize()
        st = (C.c_uint8 * n)(*([7] * n))
        bn.lib.check(bn.lib.c.wsnark_groth16_verify_batch_dev(vkb, len(vkb), d_in.data_ptr() if F.n_public else None, F.n_public, d_pr.data_ptr(), n, st, None))
        assert list(st) == [c["want"] for c in mixed], [(c["label"], g) for c, g in zip(mixed, st) if g != c["want"]]
        ones += sum(st)
    assert ones == vb.PLANTED_VALID + 3 * vb.PLANTED_SOUND_KEYS


@pytest.fixture(scope="module")
def forged4096(bn):
    F = vb.Forger(bn, 3, seed=9)
    ib, pb = F.forge(4096)
    rnd = random.Random(77)
    which = sorted(rnd.sample(range(4096), 4096 // 20))          # 5 % tampered
    tp, want = vb.tamper(pb, which, rnd)
    return F, ib, tp, want


def test_4096_forged_proofs_host_and_device_pointers(bn, forged4096):
    import torch
    F, ib, tp, want = forged4096
    vkb, n = F.vk_bytes(), 4096
    expect = [want.get(i, 1) for i in range(n)]
    assert expect.count(1) == n - n // 20
    got = vb.batch_status(bn.lib, vkb, 3, ib, tp)
    assert got == expect, [(i, g, w) for i, (g, w) in enumerate(zip(got, expect)) if g != w][:10]
    # a seeded sample of 64, half of them tampered ones, against the host call
    rnd = random.Random(5)
    sample = rnd.sample(sorted(want), 32) + rnd.sample([i for i in range(n) if i not in want], 32)
    for i in sample:
        assert vb.host_status(bn.lib, vkb, 3, ib[96 * i:96 * i + 96], tp[384 * i:384 * i + 384]) == got[i], i
    # the same buffers resident on the device
    d_in = torch.frombuffer(bytearray(ib), dtype=torch.uint8).cuda()
    d_pr = torch.frombuffer(bytearray(tp), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    st = (C.c_uint8 * n)()
    bn.lib.check(bn.lib.c.wsnark_groth16_verify_batch_dev(vkb, len(vkb), d_in.data_ptr(), 3, d_pr.data_ptr(), n, st, None))
    assert list(st) == got


def test_proofs_of_the_gpu_prover(bn):
    from wasmsnark_amd import synth
    circ = synth.make_circuit(12, n_public=2, seed=4)
    S = synth.setup(circ, seed=40)
    pkey, vk = synth.build_key(circ, S, bn.mul_base)
    key = bn.load_key(pkey)
    wit, pub = synth.witness_bin(circ), synth.public_signals(circ)
    proofs = [bn.groth16GenProof(wit, key, r=bytes([i + 1]) * 32, s=bytes([200 - i]) * 32) for i in range(16)]
    assert len({p["pi_a"][0] for p in proofs}) == 16
    assert bn.groth16Verify(vk, pub, proofs[0]) is True
    assert bn.groth16VerifyBatch(vk, [pub] * 16, proofs) == [True] * 16
    wrong = [str((int(pub[0]) + 1) % vb.R)] + pub[1:]
    assert bn.groth16VerifyBatch(vk, [wrong] * 16, proofs) == [False] * 16
    # a batch on one lane beside a proof on the other: neither result changes
    F = vb.Forger(bn, 2, seed=13)
    ib, pb = F.forge(512)
    ref = vb.batch_status(bn.lib, F.vk_bytes(), 2, ib, pb)
    assert ref == [1] * 512
    out = {}

    def prove():
        out["proof"] = bn.groth16GenProof(wit, key, r=bytes([1]) * 32, s=bytes([200]) * 32)

    t = threading.Thread(target=prove)
    t.start()
    out["status"] = vb.batch_status(bn.lib, F.vk_bytes(), 2, ib, pb)
    t.join()
    assert out["status"] == ref and out["proof"] == proofs[0]
    key.free()


def test_two_batches_from_two_threads(bn, forged4096):
    F, ib, tp, want = forged4096
    vkb = F.vk_bytes()
    halves = [(ib[:96 * 1000], tp[:384 * 1000]), (ib[96 * 1000:96 * 2500], tp[384 * 1000:384 * 2500])]
    alone = [vb.batch_status(bn.lib, vkb, 3, i, p) for i, p in halves]
    assert alone[0] + alone[1] == [want.get(i, 1) for i in range(2500)]
    res = [None, None]

    def run(k):
        res[k] = vb.batch_status(bn.lib, vkb, 3, *halves[k])

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res == alone
