// tests/iofuzz/io_formats_main.cpp -- the two file readers of pcreg_amd/csrc/io_formats.hip as a stand-alone host program, for
// tests/test_io_formats_malformed.py.  Linked with io_formats.hip and nothing else of the library (pcreg::set_error is this
// file's own); it never touches HIP.  Built with the address and undefined-behaviour sanitizers where the toolchain links them.
//
// usage: io_formats_main [--name NAME]... FILE...        the names go with every .mat file of the command line
//        io_formats_main --list LIST                     LIST: one file per line, "PATH" or "PATH<tab>NAME<tab>NAME..."
//
// For every file it does what pcreg_amd/io.py does and prints ONE line of tab-separated fields; the path comes first and is
// flushed before the first call, so that a crash names its file:
//   .pcd   PATH  call=info rc=R [n=N rgb=H | msg=M]  call=read rc=R [bytes=B sum=S | msg=M]      (or call=read skipped=cap)
//   .mat   PATH  { call=shape name=NAME rc=R [rows=R cols=C | msg=M]  call=data name=NAME rc=R [bytes=B sum=S | msg=M] }...
// once with the empty name and once per given name.  The buffers are allocated to exactly what the first call reported (ld = n),
// so that a reader writing past what it announced is caught; sum is the 64-bit FNV-1a hash of the returned bytes (xyz, then rgb).
// Messages have every byte outside printable ASCII, and the backslash, written as \xNN.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pcreg.h"

namespace pcreg {
static char g_err[1024];
void set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace pcreg

namespace {

constexpr long kMaxPoints = 4000000;          // a count above this is reported, not allocated
constexpr long kMaxElems = 16000000;          // the same for a matrix

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
constexpr uint64_t kFnvBasis = 14695981039346656037ull;

void print_msg() {
    std::fputs("\tmsg=", stdout);
    for (const char* c = pcreg::g_err; *c; ++c) {
        const unsigned char u = (unsigned char)*c;
        if (u < 32 || u > 126 || u == '\\') std::printf("\\x%02X", u); else std::fputc(u, stdout);
    }
}

bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = std::strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

void run_pcd(const char* path) {
    int n = -12345, has = -12345;
    pcreg::g_err[0] = 0;
    int rc = pcreg_pcd_info(path, &n, &has);
    std::printf("\tcall=info\trc=%d", rc);
    if (rc != PCREG_OK) { print_msg(); return; }
    std::printf("\tn=%d\trgb=%d", n, has);
    if (n < 0 || n > kMaxPoints) { std::printf("\tcall=read\tskipped=cap"); return; }
    std::fflush(stdout);
    const size_t xyz_bytes = (size_t)n * 3 * sizeof(float), rgb_bytes = has ? (size_t)n * sizeof(uint32_t) : 0;
    float* xyz = (float*)std::malloc(xyz_bytes ? xyz_bytes : 1);         // the library wants a pointer even for no point
    uint32_t* rgb = has ? (uint32_t*)std::malloc(rgb_bytes ? rgb_bytes : 1) : nullptr;
    if (!xyz || (has && !rgb)) { std::printf("\tcall=read\tskipped=alloc"); std::free(xyz); std::free(rgb); return; }
    std::memset(xyz, 0xA5, xyz_bytes);
    if (rgb) std::memset(rgb, 0xA5, rgb_bytes);
    pcreg::g_err[0] = 0;
    rc = pcreg_pcd_read(path, xyz, n, rgb, n);
    std::printf("\tcall=read\trc=%d", rc);
    if (rc != PCREG_OK) print_msg();
    else {
        uint64_t h = fnv1a(kFnvBasis, xyz, xyz_bytes);
        h = fnv1a(h, rgb, rgb_bytes);
        std::printf("\tbytes=%zu\tsum=%016llx", xyz_bytes + rgb_bytes, (unsigned long long)h);
    }
    std::free(xyz); std::free(rgb);
}

void run_mat(const char* path, const std::string& name) {
    int rows = -12345, cols = -12345;
    pcreg::g_err[0] = 0;
    int rc = pcreg_mat_read_double(path, name.empty() ? nullptr : name.c_str(), nullptr, &rows, &cols);
    std::printf("\tcall=shape\tname=%s\trc=%d", name.c_str(), rc);
    if (rc != PCREG_OK) { print_msg(); return; }
    std::printf("\trows=%d\tcols=%d", rows, cols);
    if (rows < 0 || cols < 0 || (long)rows * cols > kMaxElems) { std::printf("\tcall=data\tname=%s\tskipped=cap", name.c_str()); return; }
    std::fflush(stdout);
    const size_t bytes = (size_t)rows * cols * sizeof(double);
    double* out = (double*)std::malloc(bytes ? bytes : 1);
    if (!out) { std::printf("\tcall=data\tname=%s\tskipped=alloc", name.c_str()); return; }
    std::memset(out, 0xA5, bytes);
    int r2 = -12345, c2 = -12345;
    pcreg::g_err[0] = 0;
    rc = pcreg_mat_read_double(path, name.empty() ? nullptr : name.c_str(), out, &r2, &c2);
    std::printf("\tcall=data\tname=%s\trc=%d", name.c_str(), rc);
    if (rc != PCREG_OK) print_msg();
    else std::printf("\trows=%d\tcols=%d\tbytes=%zu\tsum=%016llx", r2, c2, bytes, (unsigned long long)fnv1a(kFnvBasis, out, bytes));
    std::free(out);
}

void run_file(const std::string& path, const std::vector<std::string>& names) {
    std::fputs(path.c_str(), stdout);
    std::fflush(stdout);
    if (ends_with(path, ".pcd")) run_pcd(path.c_str());
    else if (ends_with(path, ".mat")) {
        run_mat(path.c_str(), "");
        for (const std::string& nm : names) run_mat(path.c_str(), nm);
    } else std::fputs("\tcall=none\tskipped=suffix", stdout);
    std::fputc('\n', stdout);
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> names;
    int seen = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg == "--name" && a + 1 < argc) names.push_back(argv[++a]);
        else if (arg == "--list" && a + 1 < argc) {
            std::FILE* f = std::fopen(argv[++a], "rb");
            if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
            std::string line; int ch;
            for (;;) {
                ch = std::fgetc(f);
                if (ch != '\n' && ch != EOF) { line.push_back((char)ch); continue; }
                if (!line.empty()) {
                    std::vector<std::string> part;
                    size_t at = 0;
                    for (;;) {
                        const size_t tab = line.find('\t', at);
                        part.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at));
                        if (tab == std::string::npos) break;
                        at = tab + 1;
                    }
                    run_file(part[0], std::vector<std::string>(part.begin() + 1, part.end()));
                    ++seen;
                }
                line.clear();
                if (ch == EOF) break;
            }
            std::fclose(f);
        } else { run_file(arg, names); ++seen; }
    }
    if (!seen) { std::fprintf(stderr, "usage: %s [--name NAME]... FILE... | --list LIST\n", argv[0]); return 2; }
    return 0;
}
