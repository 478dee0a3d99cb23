// mech_pack_dump -- the host mechanism compiler and the table packer on their own (no HIP, no GPU):
// parse the mechanism files, pack them, and write every table as <out_dir>/<name>.bin (raw bytes) and the
// scalar fields of the DevMech block as name=value lines in <out_dir>/devmech.txt. The CPU tests compare
// these with tests/golden/packed_tables.json and decode them against the br_mech_desc tables.
//   mech_pack_dump [--no-spread] [--no-jfast] <out_dir> <therm.dat> <gas mechanism | -> [<surface xml | -> [gasphase]]
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mech_pack.hpp"

static std::string g_err;
// what mech_host.cpp takes from the library: its error channel, and the device half of br_mech_compile,
// which does not exist here
extern "C" void br_set_last_error(const char* msg) { g_err = msg; }
extern "C" int br_mech_create(const br_mech_desc*, int, br_mech**) { return BR_ERR_UNSUPPORTED; }

template <class T>
static bool write_bin(const std::string& dir, const char* name, const std::vector<T>& v) {
    const std::string path = dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return false; }
    const size_t nw = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
    return (fclose(f) == 0) & (nw == v.size());
}

int main(int argc, char** argv) {
    brhip::PackOpts po;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--no-spread")) po.spread = false;
        else if (!strcmp(argv[i], "--no-jfast")) po.allow_jfast = false;
        else pos.push_back(argv[i]);
    }
    if (pos.size() < 3 || pos.size() > 5) {
        fprintf(stderr, "usage: mech_pack_dump [--no-spread] [--no-jfast] <out_dir> <therm.dat> <gas | -> [<surface | -> [gasphase]]\n");
        return 2;
    }
    auto opt = [&](size_t i) -> const char* { return i < pos.size() && strcmp(pos[i], "-") ? pos[i] : nullptr; };
    const std::string dir = pos[0];
    br_host_mech* h = nullptr;
    if (br_mech_parse(opt(2), pos[1], opt(3), opt(4), BR_CONV_REFERENCE, &h)) {
        fprintf(stderr, "br_mech_parse: %s\n", g_err.c_str());
        return 1;
    }
    br_mech_desc d;
    br_host_mech_desc(h, &d);
    brhip::PackedMech p;
    std::string err;
    const int rc = (d.ng <= 0 || d.ng + d.ns > 72) ? BR_ERR_UNSUPPORTED : brhip::mech_pack(&d, po, &p, &err);
    br_host_mech_free(h);
    if (rc) {
        fprintf(stderr, "mech_pack: %d %s\n", rc, err.c_str());
        return 1;
    }
    bool ok = write_bin(dir, "img", p.img) & write_bin(dir, "nasa", p.nasa) & write_bin(dir, "g_par", p.g_par) &
              write_bin(dir, "g_dnu", p.g_dnu) & write_bin(dir, "fo_par", p.fo_par) & write_bin(dir, "s_par", p.s_par) &
              write_bin(dir, "tb_eff", p.tb_eff) & write_bin(dir, "col_ptr", p.col_ptr) & write_bin(dir, "col_rx", p.col_rx) &
              write_bin(dir, "g_perm", p.g_perm);
    FILE* f = fopen((dir + "/devmech.txt").c_str(), "w");
    if (!f) return 1;
    const brhip::DevMech& M = p.dm;
#define I_(x) fprintf(f, #x "=%d\n", M.x)
    I_(ng); I_(ns); I_(n); I_(nrg); I_(nrs); I_(ntb); I_(nfo); I_(ntbe); I_(nset); I_(conv); I_(nu4); I_(cpl);
    fprintf(f, "p_std=%.17g\nG=%.17g\n", M.p_std, M.G);
    I_(img_bytes); I_(sx_off); I_(sxe_off); I_(tbe_off); I_(tbs_off); I_(fod_off); I_(skd_off); I_(rblock_bytes);
    I_(jfast); I_(ntbr); I_(cmp_off); I_(cmr_off); I_(tjp_off); I_(tje_off);
#undef I_
    ok &= fclose(f) == 0;
    return ok ? 0 : 1;
}
