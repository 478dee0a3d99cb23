// mech_pack.hpp -- the host-side table packer of br_mech_create: br_mech_desc -> the DevMech block and
// the tables the kernels read (brhip_layout.hpp has the formats). Plain host C++: no HIP call, no I/O,
// no environment.
#pragma once
#include <string>
#include <vector>

#include "../../include/brhip.h"
#include "brhip_layout.hpp"

namespace brhip {

struct PackOpts {
    bool spread = true;        // permute the scatter lists against LDS address conflicts (spread_slots)
    bool allow_jfast = true;   // build the gas-only fast Jacobian's lists where the mechanism is eligible
};

struct PackedMech {
    DevMech dm{};              // every scalar field filled, every pointer null
    std::vector<uint4> img;    // LDS table image, dm.img_bytes
    std::vector<double> nasa, g_par, fo_par, s_par, tb_eff;
    std::vector<int> g_dnu, col_ptr, col_rx;
    std::vector<int> g_perm;   // [nrg] gas reaction of br_mech_desc at each packed (evaluation-order) position:
                               // a per-reaction array in the caller's order (br_opts.rate_mult) is read through it
};

// d: sizes checked by the caller (ng > 0, the others >= 0, ng + ns <= 72).
// Returns 0, or a BR_ERR_* code with its message in *err.
int mech_pack(const br_mech_desc* d, const PackOpts& opts, PackedMech* out, std::string* err);

}  // namespace brhip
