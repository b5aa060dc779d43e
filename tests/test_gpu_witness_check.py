"""-m gpu: the witness check (wsnark_witness_check, wsnark_circuit_load / _witness_check / _witness_check_dev, csrc/witcheck.hip) of the
hipcc-built libwsnark.so on the device.  The checks of tests/test_emul_witness_check.py again (tests/witness_check_common.py holds them
and their yardstick): 2^4 is less than a wavefront, 2^6 exactly one, 2^10 four 256-lane workgroups and sixteen words of the bitmask;
and the variant that takes the witness where it already is."""
import pytest

import witness_check_common as wc

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
@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_good_witnesses_pass(bn, log_domain, style):
    wc.check_good(bn, log_domain, style)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_planted_failures_give_exactly_the_python_set(bn, log_domain):
    wc.check_planted(bn, log_domain)


def test_truncated_lists_and_every_verdict_of_the_hand_built_circuit(bn):
    wc.check_truncation(bn, 6)


def test_unreduced_signals(bn):
    wc.check_unreduced(bn, 6)


def test_a_longer_witness_buffer_is_accepted(bn):
    wc.check_longer_buffer(bn, 4)


def test_errors_leave_the_report_and_the_lists_untouched(bn):
    wc.check_errors(bn, bn.lib.path, 4)


def test_one_handle_two_threads(bn):
    wc.check_two_threads(bn, 6)


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_the_witness_already_on_the_device(bn, log_domain):
    wc.check_dev_variant(bn, log_domain)


@pytest.mark.parametrize("dev", [False, True])
def test_gen_proof_checks_the_witness_first(bn, dev):
    wc.check_gen_proof(bn, 6, dev=dev)
