// mech_pack.cpp -- br_mech_desc -> DevMech + packed tables (see mech_pack.hpp; formats in brhip_layout.hpp)
#include "mech_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace brhip {
namespace {

uint32_t pack4(const int* v, int cnt, int pad = 255) {
    uint32_t w = 0;
    for (int e = 0; e < 4; ++e) w |= (uint32_t)(e < cnt ? (v[e] & 255) : pad) << (8 * e);
    return w;
}

// net-stoichiometry scatter list of a reaction: up to 6 (species, nu != 0) pairs packed in
// 4 words (brhip_layout.hpp sl_put / sl_off / sl_nu)
bool scatter_pack(const int* f, int nf, const int* pr, int np, uint32_t* w) {
    int sp[12], nu[12], c = 0;
    auto add = [&](int k, int v) {
        for (int i = 0; i < c; ++i) if (sp[i] == k) { nu[i] += v; return; }
        sp[c] = k; nu[c] = v; ++c;
    };
    for (int e = 0; e < nf; ++e) add(f[e], -1);
    for (int e = 0; e < np; ++e) add(pr[e], 1);
    int mm = 0;
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int i = 0; i < c; ++i) {
        if (nu[i] == 0) continue;
        if (mm >= 6 || nu[i] < -8 || nu[i] > 7 || sp[i] < 0 || sp[i] > 255) return false;
        sl_put(w, mm, sp[i], nu[i]);
        ++mm;
    }
    w[3] |= (uint32_t)mm << 24;
    return true;
}

// ---- scatter-slot order: the production sums are accumulated with one LDS atomic instruction per
//      list slot e over the 64 reactions of a pass (lanes), so a species that sits in the same
//      slot of many of those reactions serialises that instruction (LDS address conflicts; GRI's
//      H, O, OH, H2O ...). Per group of 64 reactions, each reaction's list is permuted so that its
//      species land in the slots where they are least used so far (greedy, exhaustive over the
//      <= 720 orders of one list). Only the order of the per-species sums changes.
void spread_slots(std::vector<uint32_t>& recs, int words, int off, int nrec) {
    for (int g0 = 0; g0 < nrec; g0 += WAVE) {
        static thread_local int cnt[6][256];
        memset(cnt, 0, sizeof(cnt));
        for (int i = g0; i < std::min(nrec, g0 + WAVE); ++i) {
            uint32_t* w = &recs[(size_t)words * i + off];
            const int m = (int)(w[3] >> 24);
            int sp[6], nu[6], ord[6], best[6];
            for (int e = 0; e < m; ++e) {
                sp[e] = (int)(sl_off(w[e >> 1], e & 1) >> 3);
                nu[e] = sl_nu(w[3], e);
                ord[e] = e;
            }
            long bc = -1;
            do {   // ord[slot] = entry placed in that slot
                long c = 0;
                for (int t = 0; t < m; ++t) { const long v = cnt[t][sp[ord[t]]] + 1; c += v * v; }
                if (bc < 0 || c < bc) { bc = c; std::copy(ord, ord + m, best); }
            } while (std::next_permutation(ord, ord + m));
            uint32_t nw[4] = {0, 0, 0, w[3] & 0xFF000000u};
            for (int t = 0; t < m; ++t) {
                const int e = best[t];
                sl_put(nw, t, sp[e], nu[e]);
                cnt[t][sp[e]]++;
            }
            for (int q = 0; q < 4; ++q) w[q] = nw[q];
        }
    }
}

}  // namespace

int mech_pack(const br_mech_desc* d, const PackOpts& opts, PackedMech* out, std::string* err) {
    auto fail = [err](int code, const char* msg) { *err = msg; return code; };
    const int ng = d->ng, ns = d->ns, nrg = d->nrg, nrs = d->nrs, n = ng + ns;
    *out = PackedMech();
    DevMech& M = out->dm;
    M.ng = ng; M.ns = ns; M.n = n; M.nrg = nrg; M.nrs = nrs; M.conv = d->conv;
    M.cpl = n > 64 ? 2 : 1;
    const int SPW = M.cpl == 2 ? Lay<2>::SPW : Lay<1>::SPW;       // species slots
    const int SP_ONE = M.cpl == 2 ? Lay<2>::ONE : Lay<1>::ONE;    // pad species: conc = 1
    const int IMG_RX_OFF = M.cpl == 2 ? Lay<2>::IMG_RX : Lay<1>::IMG_RX;
    M.p_std = d->p_std > 0 ? d->p_std : 1e5;
    M.G = d->site_density * 1e4;
    // ---- gas reactions, evaluated in a permuted order (falloff, then +M, then elementary) so
    //      that the lanes of one pass take the same branch; results are per species, so the
    //      order is invisible outside the kernel
    std::vector<int> perm;
    for (int pass = 2; pass >= 0; --pass)
        for (int r = 0; r < nrg; ++r) if (d->g_tb[r] == pass) perm.push_back(r);
    out->g_perm = perm;
    int ntb = 0, nfo = 0;
    for (int i = 0; i < nrg; ++i) {
        if (d->g_tb[perm[i]] == 2) nfo++;
        if (d->g_tb[perm[i]]) ntb++;
    }
    if (ntb > 1023 || nfo > 1023) return fail(BR_ERR_UNSUPPORTED, "too many third-body reactions");
    std::vector<uint32_t> rx(RX_WORDS * (size_t)nrg, 0);
    std::vector<double>& gpar = out->g_par;
    std::vector<double>& fopar = out->fo_par;
    std::vector<int>& gdnu = out->g_dnu;
    gpar.assign(4 * (size_t)std::max(nrg, 1), 0.0);
    fopar.assign(8 * (size_t)std::max(nfo, 1), 0.0);
    gdnu.assign(std::max(nrg, 1), 0);
    std::vector<std::pair<int, double>> tbe;       // (species, eff - 1), per set
    std::vector<std::vector<double>> sets;         // distinct efficiency rows
    std::vector<uint32_t> tbs;                     // per set: start | count << 20
    std::vector<double>& tbeff = out->tb_eff;      // dense [nset][n]
    int foi = 0;
    for (int i = 0; i < nrg; ++i) {
        const int r = perm[i];
        const int nf = d->g_nf[r], nr = d->g_nr[r], tb = d->g_tb[r];
        if (nf > 4 || nr > 4 || nf < 1) return fail(BR_ERR_UNSUPPORTED, "reaction with >4 entries");
        uint32_t* rec = &rx[RX_WORDS * (size_t)i];
        rec[0] = pack4(d->g_f + r * 4, nf, SP_ONE);
        rec[1] = pack4(d->g_r + r * 4, nr, SP_ONE);
        if (!scatter_pack(d->g_f + r * 4, nf, d->g_r + r * 4, nr, rec + 4))
            return fail(BR_ERR_UNSUPPORTED, "reaction touches more than 6 species");
        for (int c = 0; c < 3; ++c) gpar[4 * (size_t)i + c] = d->g_arr[r * 3 + c];
        gpar[4 * (size_t)i + 3] = (d->conv & BR_CONV_KC_UNIT_SLIP) ? std::pow(1e6, (double)(nr - nf)) : 1.0;
        gdnu[i] = nr - nf;
        int troe = 0, fo = 0, tbidx = 0;
        if (tb) {   // third-body efficiency set (deduplicated: GRI's 41 reactions use 10 sets)
            std::vector<double> row(d->g_eff + (size_t)r * ng, d->g_eff + (size_t)r * ng + ng);
            int sidx = -1;
            for (size_t q = 0; q < sets.size(); ++q) if (sets[q] == row) { sidx = (int)q; break; }
            if (sidx < 0) {
                sidx = (int)sets.size();
                sets.push_back(row);
                const int start = (int)tbe.size();
                for (int k = 0; k < ng; ++k) if (row[k] != 1.0) tbe.push_back({k, row[k] - 1.0});
                const int cnt = (int)tbe.size() - start;
                if (start >= (1 << 20) || cnt >= (1 << 12)) return fail(BR_ERR_UNSUPPORTED, "third-body list too long");
                tbs.push_back((uint32_t)start | ((uint32_t)cnt << 20));
                for (int k = 0; k < n; ++k) tbeff.push_back(k < ng ? row[k] : 0.0);
            }
            tbidx = sidx;
        }
        if (tb == 2) {
            fo = foi++;
            troe = d->g_troe_n[r];
            for (int c = 0; c < 3; ++c) fopar[8 * (size_t)fo + c] = d->g_low[r * 3 + c];
            for (int c = 0; c < 4; ++c) fopar[8 * (size_t)fo + 3 + c] = d->g_troe[r * 4 + c];
            fopar[8 * (size_t)fo + 7] = troe;
        }
        rec[2] = (uint32_t)(nf | (nr << 3) | ((d->g_rev[r] ? 1 : 0) << 6) | (tb << 7) | ((troe & 7) << 9) |
                            (fo << 12) | (tbidx << 22));
    }
    M.ntb = ntb; M.nfo = nfo; M.ntbe = (int)tbe.size(); M.nset = (int)sets.size();
    M.nu4 = 0;
    for (int r = 0; r < nrg; ++r) if (d->g_nf[r] > 3 || d->g_nr[r] > 3) M.nu4 = 1;
    if (M.nset > 64) return fail(BR_ERR_UNSUPPORTED, "more than 64 third-body efficiency sets");
    // ---- surface reactions
    std::vector<uint32_t> sx(SX_WORDS * (size_t)nrs, 0);
    std::vector<double> sxe(SXE_DOUBLES * (size_t)nrs, 0.0);
    std::vector<double>& spar = out->s_par;
    spar.assign(4 * (size_t)std::max(nrs, 1), 0.0);
    for (int r = 0; r < nrs; ++r) {
        const int nf = d->s_nf[r], np = d->s_np[r], nc = d->s_ncov[r];
        if (nf > 6 || np > 6 || nc > 4) return fail(BR_ERR_UNSUPPORTED, "surface reaction too large");
        uint32_t* rec = &sx[SX_WORDS * (size_t)r];
        int e6[6];
        for (int e = 0; e < 6; ++e) e6[e] = e < nf ? d->s_f[r * 6 + e] : SP_ONE;
        rec[0] = pack4(e6, 4);
        rec[1] = pack4(e6 + 4, 2, SP_ONE);
        // constant site factor of the rate: Gamma/sigma per surface reactant (concentration
        // theta*Gamma/sigma), 1 for gas reactants and for sticking reactions (theta only)
        double fold = 1.0;
        for (int e = 0; e < nf; ++e) {
            const int sp = d->s_f[r * 6 + e];
            if (sp >= ng && !d->s_stick[r]) fold *= M.G / (d->sigma ? d->sigma[sp - ng] : 1.0);
        }
        sxe[SXE_DOUBLES * (size_t)r + 4] = fold;
        int p6[6];
        for (int e = 0; e < 6; ++e) p6[e] = e < np ? d->s_p[r * 6 + e] : 255;
        rec[2] = pack4(p6, 4);
        rec[3] = pack4(p6 + 4, 2);
        if (!scatter_pack(d->s_f + r * 6, nf, d->s_p + r * 6, np, rec + 6))
            return fail(BR_ERR_UNSUPPORTED, "surface reaction touches more than 6 species");
        int cs[4] = {0, 0, 0, 0};
        for (int c = 0; c < nc; ++c) { cs[c] = d->s_cov_sp[r * 4 + c]; sxe[SXE_DOUBLES * (size_t)r + c] = d->s_cov_eps[r * 4 + c]; }
        rec[5] = pack4(cs, 4);
        int g = -1;
        for (int e = 0; e < nf; ++e) if (d->s_f[r * 6 + e] < ng) g = d->s_f[r * 6 + e];
        if (d->s_stick[r] && g < 0) return fail(BR_ERR_INPUT, "sticking reaction without gas reactant");
        rec[4] = (uint32_t)(nf | (np << 3) | ((d->s_stick[r] ? 1 : 0) << 6) | (nc << 7) | ((g < 0 ? 0 : g) << 10));
        for (int c = 0; c < 3; ++c) spar[4 * (size_t)r + c] = d->s_arr[r * 3 + c];
        spar[4 * (size_t)r + 3] = g >= 0 ? d->molwt[g] : 1.0;
    }
    if (opts.spread) {   // (off: lists in first-appearance order, A/B)
        spread_slots(rx, RX_WORDS, 4, nrg);
        spread_slots(sx, SX_WORDS, 6, nrs);
    }
    // ---- Jacobian column lists: reactions whose rate depends on component j
    std::vector<int>& colptr = out->col_ptr;
    std::vector<int>& colrx = out->col_rx;
    colptr.assign(1, 0);
    for (int j = 0; j < n; ++j) {
        for (int i = 0; i < nrg; ++i) {
            const int r = perm[i];
            bool dep = false;
            for (int e = 0; e < d->g_nf[r]; ++e) dep |= d->g_f[r * 4 + e] == j;
            for (int e = 0; e < d->g_nr[r]; ++e) dep |= d->g_r[r * 4 + e] == j;
            if (d->g_tb[r] && j < ng && d->g_eff[(size_t)r * ng + j] != 0.0) dep = true;
            if (dep) colrx.push_back(i);
        }
        for (int r = 0; r < nrs; ++r) {
            bool dep = false;
            for (int e = 0; e < d->s_nf[r]; ++e) dep |= d->s_f[r * 6 + e] == j;
            for (int c = 0; c < d->s_ncov[r]; ++c) dep |= d->s_cov_sp[r * 4 + c] == j;
            if (dep) colrx.push_back(nrg + r);
        }
        colptr.push_back((int)colrx.size());
    }
    // ---- gas-only fast Jacobian (jacobian_fast): reactant / product column lists (no third-body
    //      entries: that dependence goes through the efficiency sets), staged in the LDS image
    std::vector<int> cmp(1, 0);
    std::vector<uint16_t> cmr;
    const bool jfast = (ns == 0) && (M.cpl == 1) && (M.nset <= JF_MAXSET) && (ntb <= WAVE) && (nrg < 65536) &&
                       opts.allow_jfast;
    if (jfast) {
        for (int j = 0; j < n; ++j) {
            for (int i = 0; i < nrg; ++i) {
                const int r = perm[i];
                bool dep = false;
                for (int e = 0; e < d->g_nf[r]; ++e) dep |= d->g_f[r * 4 + e] == j;
                for (int e = 0; e < d->g_nr[r]; ++e) dep |= d->g_r[r * 4 + e] == j;
                if (dep) cmr.push_back((uint16_t)i);
            }
            cmp.push_back((int)cmr.size());
        }
    }
    // ---- LDS table image: molwt[SPW] | sigma[SPW] | RX | SX | SXE | TBE | TBS | CMP | CMR
    auto al16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    size_t off = IMG_RX_OFF + al16(RX_WORDS * 4 * (size_t)nrg);
    M.sx_off = (int)off;
    off += al16(SX_WORDS * 4 * (size_t)nrs);
    M.sxe_off = (int)off;
    off += al16(8 * SXE_DOUBLES * (size_t)nrs);
    M.tbe_off = (int)off;
    off += al16(16 * tbe.size());
    M.tbs_off = (int)off;
    off += al16(4 * tbs.size());
    M.jfast = jfast ? 1 : 0;
    M.ntbr = ntb;
    M.cmp_off = (int)off;
    off += jfast ? al16(4 * cmp.size()) : 0;
    M.cmr_off = (int)off;
    off += jfast ? al16(2 * cmr.size()) : 0;
    // per gas species, the efficiency sets with eff != 1 (jacobian_fast's third-body columns)
    std::vector<int> tjp(1, 0);
    std::vector<std::pair<int, double>> tje;
    if (jfast) {
        for (int j = 0; j < n; ++j) {
            for (size_t q = 0; q < sets.size(); ++q)
                if (j < ng && sets[q][j] != 1.0) tje.push_back({(int)q, sets[q][j] - 1.0});
            tjp.push_back((int)tje.size());
        }
    }
    M.tjp_off = (int)off;
    off += jfast ? al16(4 * tjp.size()) : 0;
    M.tje_off = (int)off;
    off += jfast ? al16(16 * tje.size()) : 0;
    M.img_bytes = (int)al16(off);
    out->img.assign(M.img_bytes / 16, uint4{0, 0, 0, 0});
    {
        unsigned char* img = reinterpret_cast<unsigned char*>(out->img.data());
        double* mw = reinterpret_cast<double*>(img);
        for (int k = 0; k < SPW; ++k) { mw[k] = 1.0; mw[SPW + k] = 1.0; }
        for (int k = 0; k < ng; ++k) mw[k] = d->molwt[k];
        for (int i = 0; i < ns; ++i) mw[SPW + ng + i] = d->sigma ? d->sigma[i] : 1.0;
        if (nrg) {
            uint32_t* ra = reinterpret_cast<uint32_t*>(img + IMG_RX_OFF);
            for (int i = 0; i < nrg; ++i)
                for (int w = 0; w < RX_WORDS; ++w) ra[(w < 4 ? 4 * i : 4 * nrg + 4 * i) + (w & 3)] = rx[(size_t)RX_WORDS * i + w];
        }
        if (nrs) memcpy(img + M.sx_off, sx.data(), sx.size() * 4);
        if (nrs) memcpy(img + M.sxe_off, sxe.data(), sxe.size() * 8);
        if (!tbs.empty()) memcpy(img + M.tbs_off, tbs.data(), tbs.size() * 4);
        if (jfast) {
            memcpy(img + M.cmp_off, cmp.data(), cmp.size() * 4);
            if (!cmr.empty()) memcpy(img + M.cmr_off, cmr.data(), cmr.size() * 2);
            memcpy(img + M.tjp_off, tjp.data(), tjp.size() * 4);
            for (size_t q = 0; q < tje.size(); ++q) {
                memcpy(img + M.tje_off + 16 * q, &tje[q].first, 4);
                memcpy(img + M.tje_off + 16 * q + 8, &tje[q].second, 8);
            }
        }
        for (size_t i = 0; i < tbe.size(); ++i) {
            unsigned char* e = img + M.tbe_off + 16 * i;
            const int sp = tbe[i].first;
            memcpy(e, &sp, 4);
            memcpy(e + 8, &tbe[i].second, 8);
        }
    }
    M.fod_off = fod_off_bytes(nrg);
    M.skd_off = skd_off_bytes(nrg, nfo);
    M.rblock_bytes = rblock_bytes(nrg, nfo, nrs, M.cpl);
    out->nasa.assign(d->nasa, d->nasa + (size_t)ng * 15);
    if (tbeff.empty()) tbeff.push_back(0.0);
    if (colrx.empty()) colrx.push_back(0);
    return 0;
}

}  // namespace brhip
