"""CPU: the contract table of the radix-2^29 field (tests/field29_contracts.py) through the C bodies of field29.h -- as kernels under
the thread emulator (impl 0: Field29<P>, impl 3: Field29I<Fq>) and as plain host calls (impl 2) -- with raw limbs at the operand bounds
the contracts allow.  The device's generated multiply-add chains are judged by tests/test_gpu_field29_contracts.py on the same table."""
import pytest

import field29_contracts as fc
from emul_util import emul_bn128

LEGS = [(0, 0), (0, 2), (0, 3), (1, 0), (1, 2)]


@pytest.fixture(scope="module")
def bn():
    return emul_bn128()


@pytest.mark.parametrize("which,impl,name", [(w, i, n) for w, i in LEGS for n in fc.rows_for(w, i)],
                         ids=lambda v: v if isinstance(v, str) else str(v))
def test_field29_contract(bn, which, impl, name):
    fc.check_row(bn, which, impl, name)


@pytest.mark.parametrize("which,impl", LEGS)
def test_field29_zero_lands_on_its_representatives(bn, which, impl):
    fc.check_zero_representatives(bn, which, impl)


def test_field29_unknown_arguments_are_errors(bn):
    fc.check_argument_errors(bn)


def test_field29_table_covers_every_op():
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "wsnark.h")).read()
    ops = {int(v) for v in re.findall(r"WSNARK_F29_[A-Z0-9_]+ = (\d+)", hdr)}
    assert ops == set(range(39)) == {r.op for r in fc.ROWS}
