"""-m gpu: the batch prover (wsnark_groth16_prove_batch[_dev], csrc/provebatch.hip) of the hipcc-built libwsnark.so on the device.  The
checks of tests/test_emul_prove_batch.py again (tests/prove_batch_common.py holds them; the yardstick is the single prover on the same
handle, byte for byte): 2^4 is less than a wavefront of points, 2^6 exactly one, at 2^10 a window's index list is four entries per
lane and the boolean-heavy witness puts half of window 0 into one bucket; and the variant that takes the witnesses where they are."""
import pytest

import prove_batch_common as pb

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


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("style", ["columns", "rows"])
@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_equals_the_single_prover(bn, log_domain, style, count):
    pb.check_equals_single(bn, log_domain, style, count)


@pytest.mark.parametrize("log_domain", [6, 10])
def test_equals_the_single_prover_65_proofs(bn, log_domain):
    pb.check_equals_single(bn, log_domain, "rows", 65)


def test_the_references_own_proofs(bn):
    pb.check_reference_proofs(bn)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_adversarial_witnesses_in_one_batch(bn, log_domain):
    pb.check_adversarial(bn, log_domain)


@pytest.mark.parametrize("log_domain", [6, 10])
def test_boolean_heavy_witness(bn, log_domain):
    pb.check_boolean_heavy(bn, log_domain)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_planted_equal_and_opposite_points(bn, log_domain):
    pb.check_planted_points(bn, log_domain)


@pytest.mark.parametrize("log_domain", [4, 10])
def test_geometry_and_routing_change_nothing(bn, log_domain):
    pb.check_geometry(bn, log_domain)


def test_drawn_blinding(bn):
    pb.check_drawn_blinding(bn, 6)


def test_errors_leave_the_outputs_and_the_report_untouched(bn):
    pb.check_errors(bn, bn.lib.path, 4)


def test_two_threads_one_handle(bn):
    pb.check_two_threads(bn, 6)


@pytest.mark.parametrize("log_domain", [4, 10])
def test_the_witnesses_already_on_the_device(bn, log_domain):
    pb.check_dev_variant(bn, log_domain)
