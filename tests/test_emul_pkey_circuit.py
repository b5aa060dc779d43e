"""The key-against-circuit check (wsnark_circuit_row_sums, wsnark_pkey_circuit_check*, csrc/pkeycircuit.hip) on the CPU thread
emulator: the kernel SOURCES compiled by g++ (tests/emul).  tests/pkey_circuit_common.py holds the checks and their yardsticks (Python
integers for the row sums; the closed form of a synthetic key, setup_key's and contribute_key's outputs as good keys; tampers that
plant valid points only); tests/test_gpu_pkey_circuit.py runs them again on the device at size.  Row sums at 2^4 and 2^6; verdicts
at 2^4 and ONE at 2^6: a verdict is about a dozen MSM calls, and an emulated MSM call takes about half a second."""
import pytest

import pkey_circuit_common as pc
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("log_domain", [4, 6])
def test_row_sums_are_the_python_sums(bn, log_domain):
    pc.check_row_sums(bn, log_domain)


def test_row_sums_errors(bn):
    pc.check_row_sums_errors(bn)


@pytest.mark.parametrize("which,forms", [("toxic", ("pkey",)), ("setup", ("file",)), ("contributed", ("sections",))])
def test_good_keys_pass(bn, tmp_path, tune, which, forms):
    pc.check_good_key(bn, tmp_path, tune, 4, "rows", which, forms=forms, no_vk=which == "contributed")


def test_good_key_whatever_the_chunk_and_the_seed(bn, tmp_path, tune):
    # 2^6 with PKCIRCUIT_CHUNK = 64: nVars = 66 makes the key's sections two chunks
    pc.check_good_key(bn, tmp_path, tune, 6, "columns", "contributed", chunks=(64,), seeds=(pc.SEED_B,))
    pc.check_good_key(bn, tmp_path, tune, 4, "columns", "toxic", chunks=(64, None), seeds=(pc.SEED_A, pc.SEED_B))


def test_empty_c_section(bn):
    pc.check_empty_c_section(bn)


@pytest.mark.parametrize("name", pc.TAMPERS)
def test_each_tamper_flips_exactly_its_bits(bn, tune, name):
    pc.check_tampers(bn, tune, 4, "columns", only=(name,))


def test_errors_leave_the_verdict_untouched(bn):
    pc.check_errors(bn, 4, SO_PATH)
