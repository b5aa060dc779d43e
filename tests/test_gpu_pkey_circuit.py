"""-m gpu: the key-against-circuit check (wsnark_circuit_row_sums, wsnark_pkey_circuit_check*, csrc/pkeycircuit.hip) of the hipcc-built
libwsnark.so on the device.  The checks of tests/test_emul_pkey_circuit.py again (tests/pkey_circuit_common.py holds them and their
yardsticks): 2^6 in the "rows" style, whose A and B2 sections hold infinity points, and 2^10 in the "columns" style -- four 256-lane
workgroups per matrix in lc_split_kernel, and 16 chunks per array with PKCIRCUIT_CHUNK = 64."""
import pytest

import pkey_circuit_common as pc

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


@pytest.mark.parametrize("log_domain", [4, 6, 10])
def test_row_sums_are_the_python_sums(bn, log_domain):
    pc.check_row_sums(bn, log_domain)


def test_row_sums_errors(bn):
    pc.check_row_sums_errors(bn)


@pytest.mark.parametrize("log_domain,style", [(6, "rows"), (10, "columns")])
@pytest.mark.parametrize("which", ["toxic", "setup", "contributed"])
def test_good_keys_pass(bn, tmp_path, tune, which, log_domain, style):
    pc.check_good_key(bn, tmp_path, tune, log_domain, style, which, forms=("pkey", "sections", "file"), no_vk=True)


@pytest.mark.parametrize("log_domain,style", [(6, "rows"), (10, "columns")])
def test_good_key_whatever_the_chunk_and_the_seed(bn, tmp_path, tune, log_domain, style):
    pc.check_good_key(bn, tmp_path, tune, log_domain, style, "contributed", chunks=(64, None), seeds=(pc.SEED_A, pc.SEED_B))


def test_empty_c_section(bn):
    pc.check_empty_c_section(bn)


@pytest.mark.parametrize("log_domain,style", [(6, "rows"), (10, "columns")])
def test_each_tamper_flips_exactly_its_bits(bn, tune, log_domain, style):
    pc.check_tampers(bn, tune, log_domain, style)


def test_errors_leave_the_verdict_untouched(bn):
    pc.check_errors(bn, 6, bn.lib.path)
