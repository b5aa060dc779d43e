"""CPU: the host's end of a proof in its new order (prove.hip: prove_assemble_early writes pi_a's bytes as soon as A is known,
prove_assemble_b pi_b's as soon as B2 and s*delta2 are, prove_assemble only pi_c's behind the last sum; the blinding's helper thread
starts from prove_msms' hook).  The proof's bytes are the same operations in another order: with injected r, s the one-call prover
gives the closed form byte for byte for two different (r, s), in the full-size arrangement (B2 known at the hook: pi_b early) and in
the small one (B2 last: pi_b in prove_assemble), on two queues and on one; and the sharded path -- groth16_prove_partial records into
groth16_prove_finish, which shares prove_assemble and never reaches the hook -- returns the one-call prover's bytes."""
import pytest

from emul_util import emul_bn128
from wasmsnark_amd import synth

RS = [(bytes(range(32)), bytes(range(32, 64))), (bytes([255] * 32), bytes(range(200, 232)))]      # (the second r is not reduced)
LOGD = 8


@pytest.fixture(scope="module")
def setup():
    bn = emul_bn128()
    circ = synth.NativeCircuit(bn.lib, LOGD, n_public=3, seed=4, style="rows")
    sec, _ = circ.build_sections()
    key = bn.load_key(sections=sec)
    yield bn, circ, sec, circ.witness_bin(), key
    key.free()


@pytest.mark.parametrize("full_size", [1, 0])
@pytest.mark.parametrize("overlap", [None, 0])
def test_injected_blinding_gives_the_closed_form(setup, tune, full_size, overlap):
    bn, circ, sec, wit, key = setup
    tune(bn.lib, "PROVE_FULL_SIZE", full_size)
    tune(bn.lib, "PROVE_OVERLAP", overlap)
    proofs = []
    for r, s in RS:
        want = circ.expected_proof(r, s)
        assert bn.groth16GenProof(wit, key, r=r, s=s) == want, (full_size, overlap)
        proofs.append(want)
    assert proofs[0] != proofs[1]
    assert all(proofs[0][k] != proofs[1][k] for k in ("pi_a", "pi_b", "pi_c"))


def test_records_path_returns_the_one_call_provers_bytes(setup, tune):
    bn, circ, sec, wit, key = setup
    tune(bn.lib, "PROVE_FULL_SIZE", 1)
    for r, s in RS:
        one_call = bn.groth16GenProof(wit, key, r=r, s=s)
        assert bn.groth16_prove_finish(key, bn.groth16_prove_partial(wit, key), r=r, s=s) == one_call
        recs = b""
        for rank in range(2):
            shard = bn.load_key(sections=sec, shard=(rank, 2))
            try:
                recs += bn.groth16_prove_partial(wit, shard, shard=(rank, 2))
            finally:
                shard.free()
        assert bn.groth16_prove_finish(key, recs, r=r, s=s) == one_call
