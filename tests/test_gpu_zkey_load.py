"""-m gpu: a snarkjs .zkey straight into a resident proving key (wsnark_pkey_load_zkey*, Bn128.load_zkey; csrc/zkey.hip: zkey_load) of
the hipcc-built libwsnark.so on the device.  The checks of tests/test_emul_zkey_load.py again (tests/zkey_load_common.py holds them
and names their yardsticks) at the sizes where the device kernels take their other paths: the H basis change's stages switch from one
twiddle per wavefront to per-lane digits between 2^7 and 2^8, and from 2^10 a stage spans more than one 256-lane workgroup."""
import pytest

import zkey_load_common as zl

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


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns"), (8, "columns"), (10, "rows")])
def test_proof_is_the_closed_form_from_bytes_and_from_a_mapped_file(bn, log_domain, style, tmp_path):
    zl.check_closed_form(bn, log_domain, style, tmp_path)


@pytest.mark.parametrize("log_domain,style", [(3, "rows"), (6, "columns"), (8, "columns"), (10, "rows")])
def test_same_handle_as_import_then_load(bn, log_domain, style):
    zl.check_same_handle(bn, log_domain, style)


@pytest.mark.parametrize("tile", [None, 256])
def test_record_order_and_corners(bn, tune, tile):
    zl.check_record_order(bn, 6, tune, tile)


@pytest.mark.parametrize("tile", [256, 2048])
def test_partition_tile_edges(bn, tune, tile):
    zl.check_tile_edges(bn, tune, tile)


@pytest.mark.parametrize("log_domain", [3, 8])
def test_h_corners(bn, log_domain):
    zl.check_h_corners(bn, log_domain)


def test_errors_leave_handle_vk_and_report_untouched(bn, tmp_path):
    zl.check_errors(bn, bn.lib.path, tmp_path)


def test_trial_proof(bn):
    zl.check_trial_proof(bn, 6)


@pytest.mark.parametrize("name", ["t3", "t6"])
def test_golden_keys(bn, name):
    zl.check_golden_key(bn, name)
