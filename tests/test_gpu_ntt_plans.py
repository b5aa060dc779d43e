"""GPU (-m gpu): the transform's digit plans on the device.  (a) The pass count forced through NTT_PASSES at sizes the oracle checks --
the grid of tests/test_emul_ntt_plans.py plus 2^17 and 2^18 in four passes.  (c) The REAL four-pass sizes 2^25 (7,6,6,6), 2^26
(7,7,6,6: the one plan whose middle digits differ) and 2^27 (7,7,7,6) on planted values against the transform's definition in plain
integers.  (d) CALC_H on the four-pass domain 2^25 against its closed form on a few non-zero rows.  (The same sizes on dense data
against the four-step route: test_four_step_ntt_building_blocks_on_gpu in tests/test_gpu_parity.py.)  Everything is bit-exact."""
import random

import pytest

import ntt_plans_common as npc

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


@pytest.mark.parametrize("passes,bits", npc.FORCED_PLANS + [(4, 17), (4, 18)])      # (5,4,4,4), (5,5,4,4)
def test_forced_plan_vs_oracle(bn, orc, tune, passes, bits):
    npc.check_forced_plan(bn, orc, tune, passes, bits)


@pytest.mark.parametrize("passes,dom_bits", npc.FORCED_CALC_H)
def test_forced_calc_h_vs_oracle(bn, orc, tune, passes, dom_bits):
    npc.check_forced_calc_h(bn, orc, tune, passes, dom_bits)


def test_switch_unset_keeps_the_default_plans(bn):
    npc.check_default_plans(bn, (12, 17))          # two and three passes (four: 2^25 below)


def _variants(bits):
    """(odd, inverse): all four; at 2^27 forward odd 0 and inverse odd 1 only -- every variant leaves a 4 GB table resident."""
    return [(0, False), (1, True)] if bits >= 27 else [(0, False), (1, False), (0, True), (1, True)]


@pytest.mark.parametrize("bits", [25, 26, 27])
def test_real_four_pass_sizes_vs_definition(bn, bits):
    """Zeros except at planted positions -- the ends, the middle, one bit inside every digit of the plan, two random ones -- and at
    least 4096 outputs (the ends, every 2^j and 2^j - 1, random ones) against ntt_sparse.  An output written to the wrong place, a
    wrong table entry or a wrong root moves nearly every output of such a vector."""
    import torch
    n = 1 << bits
    rnd = random.Random(bits)
    assert npc.default_passes(bits) == 4
    pos = npc.planted_positions(bits, rnd)
    assert len(pos) >= 9
    x = {j: rnd.randrange(1, npc.R) for j in pos}
    ks = npc.sample_indices(bits, rnd, 4096)
    d_pos = torch.tensor(pos, dtype=torch.int64, device="cuda")
    d_val = torch.frombuffer(bytearray(b"".join(npc.le(x[j]) for j in pos)), dtype=torch.uint8).view(len(pos), 32).cuda()
    d_ks = torch.tensor(ks, dtype=torch.int64, device="cuda")
    compared = 0
    for odd, inverse in _variants(bits):
        d = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d[d_pos] = d_val
        torch.cuda.synchronize()
        with npc.launches(bn.lib) as L:
            bn.fft_dev(d.data_ptr(), n, odd, inverse=inverse)
            torch.cuda.synchronize()
        assert L.passes() == (3, 1), L.counts          # the size's own plan: the switch is unset
        got = d[d_ks].cpu().numpy().tobytes()
        del d
        want = npc.ntt_sparse(bits, x, odd, inverse, ks)
        assert len(got) == 32 * len(want)
        bad = [k for i, k in enumerate(ks) if got[32 * i:32 * i + 32] != npc.le(want[i])]
        assert not bad, (bits, odd, inverse, len(bad), bad[:8])
        compared += len(want)
    assert compared == len(_variants(bits)) * len(ks) and len(ks) >= 4096
    torch.cuda.empty_cache()


def test_calc_h_2p25_four_pass_domain_vs_closed_form(bn):
    """One wsnark_calc_h on the domain 2^25, every transform of it in four passes: A non-zero on rows {0, ra, sh}, B on {sh, rb, n - 1}
    (two signals meet in ra and in rb; sh is shared), and at least 4096 outputs -- t = 0, n - 2, n - 1, every 2^j - 1, 2^j, 2^j + 1,
    random ones -- against calc_h_sparse."""
    import numpy as np
    bits = 25
    n = 1 << bits
    rnd = random.Random(2025)
    ra, rb, sh = rnd.sample(range(1, n - 1), 3)
    sig = [rnd.randrange(npc.R) for _ in range(4)]
    c = lambda: rnd.randrange(npc.R)
    pa = [[(0, c())], [(ra, c())], [(sh, c())], [(ra, c())]]
    pb = [[(n - 1, c())], [(sh, c())], [(rb, c())], [(rb, c())]]
    a_ev, b_ev = npc.row_evals(sig, pa), npc.row_evals(sig, pb)
    assert sorted(a_ev) == sorted({0, ra, sh}) and sorted(b_ev) == sorted({sh, rb, n - 1})
    A, B = npc.pols_bytes(pa), npc.pols_bytes(pb)
    out = np.empty((n, 32), dtype=np.uint8)
    with npc.launches(bn.lib) as L:
        bn.lib.check(bn.lib.c.wsnark_calc_h(b"".join(npc.le(s) for s in sig), A, len(A), B, len(B), 4, n, out.ctypes.data))
    assert L.passes() == (4 * 3, 4), L.counts
    ts = npc.sample_indices(bits, rnd, 4096, plus_minus=True)
    assert len(ts) >= 4096 and {0, n - 2, n - 1, 3, (1 << 24) + 1, (1 << 25) - 1} <= set(ts)
    got = out[np.array(ts, dtype=np.int64)].tobytes()
    want = npc.calc_h_sparse(bits, a_ev, b_ev, ts)
    assert want[-1] == 0 and ts[-1] == n - 1 and any(want)
    bad = [t for i, t in enumerate(ts) if got[32 * i:32 * i + 32] != npc.le(want[i])]
    assert not bad, (len(bad), bad[:8])
    assert not out[n - 1].any()                      # degree of A B <= 2 n - 2
