"""A snarkjs .zkey straight into a resident proving key (wsnark_pkey_load_zkey*, Bn128.load_zkey; csrc/zkey.hip: zkey_load) on the CPU
thread emulator: the kernel SOURCES compiled by g++ (tests/emul).  tests/zkey_load_common.py holds the checks and names their
yardsticks (the model .zkey, the proof's closed form, the unchanged two-step path); tests/test_gpu_zkey_load.py runs them again on the
device at size.  Keys stay at 2^3 ("rows") and 2^6 ("columns"): an emulated lane is a coroutine."""
import pytest

import zkey_load_common as zl
from emul_util import SO_PATH, emul_bn128


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns")])
def test_proof_is_the_closed_form_from_bytes_and_from_a_mapped_file(bn, log_domain, style, tmp_path):
    zl.check_closed_form(bn, log_domain, style, tmp_path)


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns")])
def test_same_handle_as_import_then_load(bn, log_domain, style):
    zl.check_same_handle(bn, log_domain, style)


@pytest.mark.parametrize("tile", [None, 256])
def test_record_order_and_corners(bn, tune, tile):
    zl.check_record_order(bn, 3, tune, tile)


@pytest.mark.parametrize("tile", [256, 2048])
def test_partition_tile_edges(bn, tune, tile):
    zl.check_tile_edges(bn, tune, tile)


def test_h_corners(bn):
    zl.check_h_corners(bn, 3)


def test_errors_leave_handle_vk_and_report_untouched(bn, tmp_path):
    zl.check_errors(bn, SO_PATH, tmp_path)


def test_trial_proof(bn):
    zl.check_trial_proof(bn, 3)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_keys(bn, name):
    zl.check_golden_key(bn, name)
