"""-m gpu: the contract table of the radix-2^29 field (tests/field29_contracts.py) on the MI355X.  On the device the four products are
not the C bodies of field29.h but the generated v_mad_u64_u32 chains of mad_chain.h, which neither the emulator nor the host ever
executes: impl 0 (Field29<P>, products as calls) and impl 3 (Field29I<Fq>, products inlined) run them with raw limbs at the operand
bounds the contracts allow, impl 2 runs the C bodies on the host of the same library, and impl 0 must equal impl 2 limb for limb
(the chains claim the same results as the bodies, not just the same residue).  A few thousand lanes per launch."""
import numpy as np
import pytest

import field29_contracts as fc

pytestmark = pytest.mark.gpu

LEGS = [(0, 0), (0, 2), (0, 3), (1, 0), (1, 2)]


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


@pytest.mark.parametrize("which", [0, 1])
def test_field29_contracts_on_device(bn, which):
    """every row on every implementation; one test per field so that the three implementations' outputs can be compared"""
    outs = {}
    for impl in (0, 2, 3):
        if (which, impl) not in LEGS:
            continue
        for name in fc.rows_for(which, impl):
            outs[impl, name] = fc.check_row(bn, which, impl, name)
    for (impl, name), out in outs.items():
        if impl != 2:
            ref = outs[2, name]
            bad = np.nonzero((out != ref).any(axis=1))[0]
            assert bad.size == 0, "%s (%s): impl %d differs from the host's C body in %d cases, first operands %s: %s / %s" % (
                name, fc.FNAME[which], impl, bad.size, [hex(x) for x in fc.cases(which, name)[0][bad[0]]], out[bad[0]].tolist(), ref[bad[0]].tolist())


@pytest.mark.parametrize("which,impl", LEGS)
def test_field29_zero_lands_on_its_representatives_on_device(bn, which, impl):
    fc.check_zero_representatives(bn, which, impl)


def test_field29_unknown_arguments_are_errors_on_device(bn):
    fc.check_argument_errors(bn)
