// brhip_layout.hpp -- what the host-side mechanism packer (mech_pack.cpp) and the device code
// (brhip_device.hpp) must agree on, and nothing else: the DevMech block, the packed record formats and
// their accessors, the species-block layout and the per-reactor LDS sizes. Plain C++: it compiles with
// the host compiler alone (-D__HIP_PLATFORM_AMD__, HIP headers for uint4 and __host__ __device__).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace brhip {

constexpr int WAVE = 64;

// ------------------------------------------------------------------------------------
// mechanism description (host-built)
// ------------------------------------------------------------------------------------
struct DevMech {
    int ng, ns, n, nrg, nrs, ntb, nfo, ntbe, nset, conv;
    int nu4;                      // some gas reaction has 4 reactants or 4 products
    int cpl;                      // components per lane: 1 (n <= 64) or 2 (64 < n <= 128), see Lay
    double p_std, G;              // Pa ; site density mol/m2
    const uint4* img;             // LDS table image (global copy)
    int img_bytes;                // multiple of 16
    int sx_off, sxe_off, tbe_off; // byte offsets in the image
    int tbs_off;                  // third-body efficiency sets: one word (start | count << 20) each
    int fod_off, skd_off;         // byte offsets of FOD / SKD from the end of the species block
    int rblock_bytes;             // per-reactor LDS bytes from SP start (SP + FOD + SKD)
    // init only (T-dependent constants)
    const double* nasa;           // [ng][15]: Tmid, a_hi[7], a_lo[7]
    const double* g_par;          // [nrg][4]: A (SI), beta, Ea/R, Kc scale
    const int* g_dnu;             // [nrg]
    const double* fo_par;         // [nfo][8]: A0, b0, E0/R, a, T***, T*, T**, ntroe
    const double* s_par;          // [nrs][4]: A or s0, beta, Ea [J/mol], M_gas (stick)
    // Jacobian only
    const double* tb_eff;         // [nset][n] dense efficiencies
    const int* col_ptr;           // [n+1] Jacobian column lists
    const int* col_rx;            // combined reaction index (gas r, surface nrg+r)
    // gas-only fast Jacobian (jfast): mass-action column lists in the LDS image (cmp_off: int
    // [n+1] column starts, cmr_off: uint16 reaction per entry; reactant / product dependence
    // only), third-body dependence through the efficiency sets (ntb third-body reactions first)
    int jfast, ntbr, cmp_off, cmr_off;
    // per gas species j, the efficiency sets with eff_j != 1: tjp_off int [n+1] starts, tje_off
    // 16-byte entries {int set, pad, double eff - 1}
    int tjp_off, tje_off;
};

// RX record: w0 reactant species (4 x 8 bit; pad = SP_ONE, a slot holding 1.0, so the
// concentration products need no branches), w1 product species, w2 info (third-body
// efficiency set in bits 22..31), w3 pad, w4..w7 net-stoichiometry scatter list (byte offsets x6
// in w4..w6, nu nibbles | count << 24 in w7; see scatter())
__host__ __device__ inline int gi_nf(uint32_t v) { return v & 7; }
__host__ __device__ inline int gi_nr(uint32_t v) { return (v >> 3) & 7; }
__host__ __device__ inline int gi_rev(uint32_t v) { return (v >> 6) & 1; }
__host__ __device__ inline int gi_tb(uint32_t v) { return (v >> 7) & 3; }
__host__ __device__ inline int gi_troe(uint32_t v) { return (v >> 9) & 7; }
__host__ __device__ inline int gi_foidx(uint32_t v) { return (v >> 12) & 1023; }
__host__ __device__ inline int gi_tbidx(uint32_t v) { return (v >> 22) & 1023; }
// SX record: w0,w1 reactants (6 x 8 bit), w2,w3 products, w4 info, w5 coverage species (4 x 8),
// w6..w9 scatter list (as RX w4..w7), w10..w11 pad
__host__ __device__ inline int si_nf(uint32_t v) { return v & 7; }
__host__ __device__ inline int si_np(uint32_t v) { return (v >> 3) & 7; }
__host__ __device__ inline int si_stick(uint32_t v) { return (v >> 6) & 1; }
__host__ __device__ inline int si_ncov(uint32_t v) { return (v >> 7) & 7; }
__host__ __device__ inline int si_gas(uint32_t v) { return (v >> 10) & 255; }
__host__ __device__ inline int sp8(uint32_t w, int e) { return (w >> (8 * e)) & 255; }
constexpr int RX_WORDS = 8, SX_WORDS = 12, SXE_DOUBLES = 8;

// Components per lane: CPL = 1 for n <= 64 (lane k <-> component k); CPL = 2 for 64 < n <= 128
// (lane k <-> components k and k + 64, e.g. GRI gas + Ni surface, n = 66). Species-indexed LDS
// arrays are sized SPW = 64 (CPL = 1) or 80 (CPL = 2, n <= 72): see Lay.
template <int CPL>
struct Lay {
    // species slots: 64, or 80 for two components per lane (n <= 72; round 3: 128 before, the LDS
    // saved per reactor lets 12 gas+surface reactors share a CU instead of 11)
    static constexpr int SPW = CPL == 2 ? 80 : 64;
    // species block (doubles): conc[SPW], conc[ONE] = 1.0 (pad species of the packed records),
    // accw[SPW], accs[SPW], mc[64] third-body concentration per efficiency set
    static constexpr int CONC = 0, ONE = SPW, ACCW = SPW + 16, ACCS = 2 * SPW + 16, MC = 3 * SPW + 16;
    static constexpr int DOUBLES = 3 * SPW + 16 + 64, BYTES = DOUBLES * 8;
    static constexpr int IMG_RX = 16 * SPW;   // image: molwt[SPW] | sigma[SPW] | RX records ...
};

__host__ __device__ inline int fod_off_bytes(int /*nrg*/) { return 0; }   // RXD is in global memory
__host__ __device__ inline int skd_off_bytes(int nrg, int nfo) { return fod_off_bytes(nrg) + 32 * nfo; }
__host__ __device__ inline int rblock_bytes(int nrg, int nfo, int nrs, int cpl) {
    return (cpl == 2 ? Lay<2>::BYTES : Lay<1>::BYTES) + skd_off_bytes(nrg, nfo) + 16 * nrs;
}

// Net-stoichiometry scatter list of a reaction (4 packed words): w0..w2 hold the byte offsets
// (species * 8) of slots 0..5, two 16-bit fields per word, w3 the 4-bit signed nu of each slot |
// count << 24. Byte offsets: a slot's address is one add of the field to the array base (a
// select-word add) instead of a byte extract and a shift-add (round 3: the production loop's
// scatter is ~1/3 of the RHS's VALU).
__host__ __device__ __forceinline__ unsigned sl_off(uint32_t w, int hi) { return hi ? (w >> 16) : (w & 0xffffu); }
__host__ __device__ __forceinline__ int sl_nu(uint32_t w3, int e) { return ((int)(w3 << (28 - 4 * e))) >> 28; }
// the packer's side: slot t of the list w[0..3] = (species sp, nu)
inline void sl_put(uint32_t* w, int t, int sp, int nu) {
    w[t >> 1] |= (uint32_t)(sp * 8) << (16 * (t & 1));
    w[3] |= (uint32_t)(nu & 15) << (4 * t);
}

// most third-body efficiency sets the gas-only fast Jacobian (DevMech::jfast) handles
constexpr int JF_MAXSET = 16;

}  // namespace brhip
