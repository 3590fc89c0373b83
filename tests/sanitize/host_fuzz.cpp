/* host_fuzz.cpp -- AddressSanitizer / UBSan harness for the host-side file readers (CPU build only: GPU sanitizers are not available on
 * the pool).  Built by tests/test_host_sanitizers.py from the product's own host sources (the readers and builders; not the context*.cpp files, which need HIP):
 *
 *   host_fuzz <seed> <mutations> file...
 *
 * (Scenes must be given as paths inside a scratch copy of their directory: damaged copies are written beside them.)
 * Every file is first read as it is (images through LoadImageRGBA32F, .pbrt / .pbf through importScene + ConvertScene + BuildBvh, .ply
 * through readPly), then `mutations` damaged copies are read: random byte flips, truncations, inserted runs and overwritten length fields.
 * A reader may succeed or report an error; it must not touch memory it does not own, overflow a signed integer or loop forever.
 * The sanitizer runtime aborts the process on a finding; the harness prints one line per file and "ok" at the end. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../tracerboy_amd/csrc/host/host_scene.h"
#include "../../tracerboy_amd/csrc/host/pbrt_scene.h"

namespace {
uint64_t rngState = 1;
uint32_t rnd() { rngState = rngState * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rngState >> 33); }

std::vector<uint8_t> slurp(const std::string& f) { std::ifstream in(f, std::ios::binary); return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>()); }
void spit(const std::string& f, const std::vector<uint8_t>& d) { std::ofstream out(f, std::ios::binary | std::ios::trunc); out.write((const char*)d.data(), (std::streamsize)d.size()); }
std::string ext(const std::string& f) { const size_t p = f.rfind('.'); std::string e = p == std::string::npos ? "" : f.substr(p); for (char& c : e) c = (char)tolower(c); return e; }

/* text files: one whitespace-delimited token replaced by something a parser may not expect, deleted or doubled */
std::vector<uint8_t> mutateToken(const std::vector<uint8_t>& src)
{
    static const char* const subst[] = {"-1", "0", "1e30", "nan", "inf", "4294967296", "-2147483649", "\"\"", "[", "]", "\"", "1e-40", "99999999999999999999", "Include", "AttributeEnd", "ObjectEnd"};
    std::vector<std::pair<size_t, size_t>> tok; size_t i = 0;
    while (i < src.size()) { while (i < src.size() && isspace(src[i])) i++; const size_t b = i; while (i < src.size() && !isspace(src[i])) i++; if (i > b) tok.push_back({b, i}); }
    if (tok.empty()) return src;
    const std::pair<size_t, size_t> t = tok[rnd() % tok.size()]; const uint32_t how = rnd() % 4;
    std::vector<uint8_t> d(src.begin(), src.begin() + (long)t.first);
    if (how == 0) { const char* r = subst[rnd() % (sizeof subst / sizeof subst[0])]; d.insert(d.end(), r, r + strlen(r)); }
    else if (how == 1) { }
    else if (how == 2) { d.insert(d.end(), src.begin() + (long)t.first, src.begin() + (long)t.second); d.push_back(' '); d.insert(d.end(), src.begin() + (long)t.first, src.begin() + (long)t.second); }
    else { const std::pair<size_t, size_t> o = tok[rnd() % tok.size()]; d.insert(d.end(), src.begin() + (long)o.first, src.begin() + (long)o.second); }
    d.insert(d.end(), src.begin() + (long)t.second, src.end());
    return d;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, bool text)
{
    std::vector<uint8_t> d = src; if (d.empty()) return d;
    if (text && rnd() % 3 != 0) { d = mutateToken(src); if (rnd() & 1) d = mutateToken(d); return d; }
    const uint32_t kind = rnd() % 6;
    if (kind == 0) { const uint32_t n = 1 + rnd() % 8; for (uint32_t i = 0; i < n; i++) d[rnd() % d.size()] ^= (uint8_t)(1u << (rnd() % 8)); }
    else if (kind == 1) d.resize(rnd() % d.size());
    else if (kind == 2) { const size_t at = rnd() % d.size(); const uint32_t n = 1 + rnd() % 64; d.insert(d.begin() + (long)at, n, (uint8_t)rnd()); }
    else if (kind == 3) { const size_t at = rnd() % d.size(); const uint8_t v[4] = {0xff, 0xff, 0xff, (uint8_t)(rnd() & 1 ? 0x7f : 0xff)}; for (size_t k = 0; k < 4 && at + k < d.size(); k++) d[at + k] = v[k]; }   /* a huge length / count */
    else if (kind == 4) { const size_t head = d.size() < 256 ? d.size() : 256; const uint32_t n = 1 + rnd() % 4; for (uint32_t i = 0; i < n; i++) d[rnd() % head] = (uint8_t)rnd(); }                                    /* headers */
    else { const size_t at = rnd() % d.size(), n = 1 + rnd() % 32; for (size_t k = 0; k < n && at + k < d.size(); k++) d[at + k] = 0; }
    return d;
}

bool readOne(const std::string& f)
{
    const std::string e = ext(f);
    try {
        if (e == ".pbrt" || e == ".pbf") {
            std::shared_ptr<tbhost::PbrtScene> s = tbhost::importScene(f); if (!s) return false;
            tbhost::HostScene hs; tbhost::ConvertOptions opt; opt.flattenInstances = (rnd() & 1) != 0; tbhost::ConvertScene(*s, hs, opt); tbhost::BuildBvh(hs, 0); return true;
        }
        if (e == ".ply") { std::vector<tbhost::Vec3> p, n; std::vector<tbhost::Vec2> uv; std::vector<uint32_t> idx; tbhost::readPly(f, p, n, uv, idx); return true; }
        std::vector<TbFloat4> texels; uint32_t w = 0, h = 0; bool norm = false, alpha = false; std::string err;
        return tbhost::LoadImageRGBA32F(f, texels, w, h, norm, err, &alpha);
    } catch (const std::exception&) { return false; }
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: host_fuzz <seed> <mutations> file...\n"); return 2; }
    rngState = strtoull(argv[1], nullptr, 10) * 2 + 1; const int mutations = atoi(argv[2]);
    char dirTemplate[] = "/tmp/tb_fuzz_XXXXXX"; const char* dir = mkdtemp(dirTemplate); if (!dir) { perror("mkdtemp"); return 2; }
    for (int a = 3; a < argc; a++) {
        const std::string f = argv[a], e = ext(f); const std::vector<uint8_t> src = slurp(f);
        const bool clean = readOne(f); int good = 0;
        /* a damaged scene is written next to the original (into a copy of its directory the caller made) so that its includes, meshes and textures still resolve */
        const bool scene = e == ".pbrt" || e == ".pbf";
        const std::string tmp = scene ? f.substr(0, f.rfind('/')) + "/tb_fuzz_mutant" + e : std::string(dir) + "/m" + e;
        for (int m = 0; m < mutations; m++) { spit(tmp, mutate(src, e == ".pbrt")); good += readOne(tmp) ? 1 : 0; }
        printf("%s: %s as it is; %d of %d damaged copies still read\n", f.c_str(), clean ? "reads" : "REFUSED", good, mutations);
        unlink(tmp.c_str());
    }
    rmdir(dir); printf("ok\n"); return 0;
}
