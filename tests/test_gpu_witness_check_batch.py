"""-m gpu: the batch witness check (wsnark_circuit_witness_check_batch[_dev], csrc/witcheck.hip) and groth16GenProofBatch[_dev](...,
circuit=rc) of the hipcc-built libwsnark.so on the device.  The checks of tests/test_emul_witness_check_batch.py again
(tests/witness_check_batch_common.py holds them and their yardsticks): 2^4 is less than a wavefront, 2^6 exactly one, 2^10 four
256-lane workgroups and sixteen mask words per witness; and the variants that take the witnesses where they already are."""
import pytest

import witness_check_batch_common as wb

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


@pytest.mark.parametrize("style", ["columns", "rows"])
@pytest.mark.parametrize("log_domain,count", [(4, 1), (4, 2), (4, 5), (4, 65), (6, 1), (6, 2), (6, 5), (6, 65), (10, 5)])
def test_equals_the_single_call_and_python(bn, log_domain, count, style):
    wb.check_equals_single(bn, log_domain, style, count)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_the_pass_size_changes_nothing(bn, log_domain):
    wb.check_geometry(bn, log_domain)


def test_stride_blob_and_sequence(bn):
    wb.check_stride(bn, 6)


def test_the_hand_built_circuit_between_two_zero_witnesses(bn):
    wb.check_hand_built(bn, 6)


def test_unreduced_signals_and_signal_0_per_witness(bn):
    wb.check_unreduced(bn, 6)


def test_errors_leave_everything_untouched(bn):
    wb.check_errors(bn, bn.lib.path, 4)


def test_two_threads_one_handle_two_batches(bn):
    wb.check_two_threads(bn, 6)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_the_witnesses_already_on_the_device(bn, log_domain):
    wb.check_dev_variant(bn, log_domain)


@pytest.mark.parametrize("dev", [False, True])
def test_the_batch_prover_checks_the_witnesses_first(bn, dev):
    wb.check_gen_proof_batch(bn, 6, dev=dev)
