// pkeycheck.h -- what the key audit (pkeycheck.hip) shares with the phase-2 contribution (pkeydelta.hip): the two cheap point tests and their
// device reduction, the fixed-point tests and the pairing relation on the host, and the rho_j of the random linear combinations.
#pragma once
#include "internal.h"
#include "fp12_host.h"

namespace wsnark {

// one section's running result; `first` holds ~(index << 3 | reason) of the smallest bad index (0 = none) so that atomicMax finds
// the minimum
struct PkAcc { unsigned long long inf, bad, first; };

struct PkSeed { uint32_t w[8]; };

__device__ inline bool pk_ge(const Fe& x, const uint64_t* m) {        // x >= m
    for (int i = 3; i >= 0; i--) {
        if (x.l[i] > m[i]) return true;
        if (x.l[i] < m[i]) return false;
    }
    return true;
}
__device__ inline bool pk_zero(const Fe& x) { return (x.l[0] | x.l[1] | x.l[2] | x.l[3]) == 0; }

// st: 0 good, 1..3 the reason, 4 infinity.  Every lane of the wavefront arrives here (lanes past the end with st = 0).
__device__ inline void pk_reduce(int st, uint64_t index, PkAcc* __restrict__ acc) {
    const unsigned long long m_inf = __ballot(st == 4), m_bad = __ballot(st >= 1 && st <= 3);
    if ((threadIdx.x & 63) == 0) {
        if (m_inf) atomicAdd(&acc->inf, (unsigned long long)__popcll(m_inf));
        if (m_bad) atomicAdd(&acc->bad, (unsigned long long)__popcll(m_bad));
    }
    if (st >= 1 && st <= 3) atomicMax(&acc->first, ~(((unsigned long long)index << 3) | (unsigned long long)st));
}

// ---- host (pkeycheck.hip) ----
// reference-format bytes -> the host pairing's point; the reason it is bad (0 = good).  check = false: only the infinity rule
uint32_t fixed_g1(const uint8_t* p, bool check, hostpair::G1A* out);
uint32_t fixed_g2(const uint8_t* p, bool check, hostpair::G2A* out);
hostpair::G1A gen1();
hostpair::G2A gen2();
bool same_log(const hostpair::G1A& P, const hostpair::G2A& Q);      // e(P, G2) == e(G1, Q)
// d_out[i] = rho_(base + i), i < n: 128 non-zero bits of the ChaCha20 block under key = seed32, counter = the global index
int pkcheck_rho_dev(Fe* d_out, uint64_t n, uint64_t base, const uint8_t* seed32, hipStream_t s);

}  // namespace wsnark
