// pcreg_amd/csrc/io_formats.cpp -- the two on-disk formats the drivers read and write:
//   .pcd  point clouds      pcread / pcwrite, completeExperimentFast.m:12-13,30,403
//   .mat  descriptor caches load, completeExperimentFast.m:21-24,312-313  (MAT-file Level 5, v6/v7)
// Host code only (no HIP): a reader so that real data can be ingested, and the PCD writer for the
// final aligned surface.  MAT v7.3 files are HDF5 and not handled here.
#include "common.hpp"
#include <zlib.h>
#include <cerrno>
#include <climits>
#include <exception>
#include <cmath>
#include <sstream>
#include <vector>

namespace pcreg {
namespace {

// ------------------------------------------------------------------------------------ PCD
// Everything in a file is untrusted: the header is validated in full before anything is sized from it, and a count is
// reported only if the file's size can back it (pcreg.h).
struct File {                                           // closes on every path out, an exception included
    FILE* f = nullptr;
    explicit File(const char* path, const char* mode) : f(fopen(path, mode)) {}
    ~File() { if (f) fclose(f); }
    File(const File&) = delete; File& operator=(const File&) = delete;
};

struct PcdField { std::string name; int size = 4; char type = 'F'; int count = 1; int offset = 0; };
struct PcdHeader {
    PcdHeader() = default;
    PcdHeader(const PcdHeader&) = delete; PcdHeader& operator=(const PcdHeader&) = delete;   // fx .. fc point into `fields`
    std::vector<PcdField> fields;
    long points = 0; long width = 0, height = 1; int point_size = 0;
    int tokens_per_point = 0;                           // the sum of the counts: what an ascii point takes
    enum { ASCII, BINARY, COMPRESSED } data = ASCII;
    long data_offset = 0, file_size = 0;
    const PcdField* fx = nullptr; const PcdField* fy = nullptr; const PcdField* fz = nullptr; const PcdField* fc = nullptr;
};

constexpr size_t kPcdMaxLine = 1 << 20;                  // a header line longer than this is no header line
constexpr int kPcdMaxPointSize = 1 << 24;

// one line of any length up to kPcdMaxLine, without its '\n': 1 = a line, 0 = end of file, -1 = too long
int pcd_read_line(FILE* f, std::string& line) {
    line.clear();
    int ch;
    while ((ch = fgetc(f)) != EOF) {
        if (ch == '\n') return 1;
        if (line.size() >= kPcdMaxLine) return -1;
        line.push_back((char)ch);
    }
    return line.empty() ? 0 : 1;
}

// the whole token as a decimal integer that fits a long
bool parse_long(const std::string& s, long& v) {
    if (s.empty() || !(s[0] == '-' || s[0] == '+' || (s[0] >= '0' && s[0] <= '9'))) return false;
    char* end = nullptr; errno = 0;
    v = strtol(s.c_str(), &end, 10);
    return errno == 0 && end == s.c_str() + s.size();
}

int pcd_bad(const char* path, const char* what) { set_error("%s: PCD header: %s", path, what); return PCREG_E_ARG; }

int pcd_parse_header(FILE* f, PcdHeader& h, const char* path) {
    std::string line;
    std::vector<std::string> names, types; std::vector<long> sizes, counts;
    bool have_points = false, have_data = false, have_counts = false;
    int got;
    while ((got = pcd_read_line(f, line)) == 1) {
        std::istringstream is(line);
        std::string key, s; is >> key;
        if (key.empty() || key[0] == '#') continue;
        auto numbers = [&](std::vector<long>& out) { out.clear(); long v; while (is >> s) { if (!parse_long(s, v)) return false; out.push_back(v); } return true; };
        auto number = [&](long& out) { return (is >> s) && parse_long(s, out); };
        if (key == "FIELDS" || key == "COLUMNS") { names.clear(); while (is >> s) names.push_back(s); }
        else if (key == "SIZE") { if (!numbers(sizes)) return pcd_bad(path, "SIZE holds something that is no number"); }
        else if (key == "TYPE") { types.clear(); while (is >> s) types.push_back(s); }
        else if (key == "COUNT") { if (!numbers(counts)) return pcd_bad(path, "COUNT holds something that is no number"); have_counts = true; }
        else if (key == "WIDTH") { if (!number(h.width)) return pcd_bad(path, "WIDTH is no number"); }
        else if (key == "HEIGHT") { if (!number(h.height)) return pcd_bad(path, "HEIGHT is no number"); }
        else if (key == "POINTS") { if (!number(h.points)) return pcd_bad(path, "POINTS is no number"); have_points = true; }
        else if (key == "DATA") {
            is >> s;
            if (s == "ascii") h.data = PcdHeader::ASCII;
            else if (s == "binary") h.data = PcdHeader::BINARY;
            else if (s == "binary_compressed") h.data = PcdHeader::COMPRESSED;
            else { set_error("%s: unknown PCD DATA kind '%.40s'", path, s.c_str()); return PCREG_E_ARG; }
            have_data = true;
            break;
        }
    }
    if (got < 0) return pcd_bad(path, "a line of more than 1 MiB");
    if (!have_data || names.empty()) { set_error("%s: not a PCD file (no FIELDS/DATA header)", path); return PCREG_E_ARG; }
    if (sizes.size() != names.size() || types.size() != names.size() || (have_counts && counts.size() != names.size()))
        return pcd_bad(path, "FIELDS/SIZE/TYPE/COUNT disagree in length");
    if (!have_counts) counts.assign(names.size(), 1);
    h.fields.reserve(names.size());                      // fx .. fc point into it
    long off = 0, tokens = 0;
    for (size_t i = 0; i < names.size(); ++i) {
        const long sz = sizes[i], cnt = counts[i];
        if (types[i].size() != 1 || !strchr("IUF", types[i][0])) return pcd_bad(path, "a TYPE other than I, U, F");
        const char t = types[i][0];
        if (t == 'F' ? (sz != 4 && sz != 8) : (sz != 1 && sz != 2 && sz != 4 && sz != 8)) return pcd_bad(path, "a SIZE its TYPE does not have (F: 4, 8; I, U: 1, 2, 4, 8)");
        if (cnt < 1 || cnt > kPcdMaxPointSize) return pcd_bad(path, "a COUNT below 1 or beyond 16 Mi");
        PcdField fd; fd.name = names[i]; fd.size = (int)sz; fd.type = t; fd.count = (int)cnt; fd.offset = (int)off;
        off += sz * cnt; tokens += cnt;
        if (off > kPcdMaxPointSize) return pcd_bad(path, "a point of more than 16 MiB");
        h.fields.push_back(fd);
        const PcdField* p = &h.fields.back();
        const bool colour = fd.name == "rgb" || fd.name == "rgba";
        if (colour && (sz != 4 || cnt != 1)) return pcd_bad(path, "rgb / rgba is not one 4-byte word");
        const PcdField** slot = fd.name == "x" ? &h.fx : fd.name == "y" ? &h.fy : fd.name == "z" ? &h.fz : nullptr;
        if (slot) { if (*slot) return pcd_bad(path, "x, y or z declared twice"); *slot = p; }
        if (colour) h.fc = p;
    }
    if (!h.fx || !h.fy || !h.fz) { set_error("%s: no x/y/z fields", path); return PCREG_E_ARG; }
    h.point_size = (int)off; h.tokens_per_point = (int)tokens;
    if (h.width < 0 || h.height < 0 || h.width > INT_MAX || h.height > INT_MAX || h.width * h.height > INT_MAX)
        return pcd_bad(path, "WIDTH / HEIGHT negative or WIDTH * HEIGHT beyond INT_MAX");
    if (!have_points) h.points = h.width * h.height;
    if (h.points < 0 || h.points > INT_MAX) return pcd_bad(path, "POINTS negative or beyond INT_MAX");
    h.data_offset = ftell(f);
    if (h.data_offset < 0 || fseek(f, 0, SEEK_END) != 0 || (h.file_size = ftell(f)) < h.data_offset || fseek(f, h.data_offset, SEEK_SET) != 0) {
        set_error("%s: cannot tell the file's size", path); return PCREG_E_ARG;
    }
    // the payload the header promises has to be there: nothing is allocated, here or by the caller, from a count the file
    // cannot back.  points <= INT_MAX and point_size <= 2^24, so the products stay far inside a long
    const long rest = h.file_size - h.data_offset, raw = h.points * h.point_size;
    if (h.data == PcdHeader::BINARY) {
        if (raw > rest) { set_error("%s: truncated binary PCD (%ld points of %d bytes, %ld bytes of payload)", path, h.points, h.point_size, rest); return PCREG_E_ARG; }
    } else if (h.data == PcdHeader::ASCII) {             // every value takes a character and, but for the last, a separator
        const long need = h.points * h.tokens_per_point * 2 - 1;
        if (h.points > 0 && need > rest) { set_error("%s: truncated ascii PCD (%ld points, %ld bytes of payload)", path, h.points, rest); return PCREG_E_ARG; }
    } else {
        uint32_t sz[2];
        if (fread(sz, 4, 2, f) != 2 || (long)sz[1] != raw || (long)sz[0] > rest - 8) { set_error("%s: bad binary_compressed sizes", path); return PCREG_E_ARG; }
        // an LZF item of 3 bytes yields 264 at the most
        if (raw > 88 * (long)sz[0]) { set_error("%s: binary_compressed PCD: %u bytes cannot hold %ld", path, sz[0], raw); return PCREG_E_ARG; }
        if (fseek(f, h.data_offset, SEEK_SET) != 0) { set_error("%s: cannot seek", path); return PCREG_E_ARG; }
    }
    return PCREG_OK;
}

// one value of a validated field as the float the caller gets: converted once, from the field's own type (an 8-byte integer
// is read as 64 bits and rounded to float directly, not by way of double)
float pcd_value(const unsigned char* p, const PcdField& f) {
    switch (f.type) {
        case 'F': if (f.size == 4) { float v; memcpy(&v, p, 4); return v; } else { double v; memcpy(&v, p, 8); return (float)v; }
        case 'U':
            switch (f.size) {
                case 1: return (float)*p;
                case 2: { uint16_t v; memcpy(&v, p, 2); return (float)v; }
                case 4: { uint32_t v; memcpy(&v, p, 4); return (float)v; }
                default: { uint64_t v; memcpy(&v, p, 8); return (float)v; }
            }
        default:
            switch (f.size) {
                case 1: return (float)*(const int8_t*)p;
                case 2: { int16_t v; memcpy(&v, p, 2); return (float)v; }
                case 4: { int32_t v; memcpy(&v, p, 4); return (float)v; }
                default: { int64_t v; memcpy(&v, p, 8); return (float)v; }
            }
    }
}

// LZF decompression (the format PCL's binary_compressed uses): control byte < 32: literal run of ctrl+1
// bytes; otherwise a back reference of length (ctrl >> 5) + 2 (7 -> +next byte) at distance
// ((ctrl & 31) << 8 | next) + 1.
bool lzf_decompress(const unsigned char* in, size_t in_len, unsigned char* out, size_t out_len) {
    size_t ip = 0, op = 0;
    while (ip < in_len) {
        unsigned ctrl = in[ip++];
        if (ctrl < 32) {
            size_t run = ctrl + 1;
            if (ip + run > in_len || op + run > out_len) return false;
            memcpy(out + op, in + ip, run); ip += run; op += run;
        } else {
            size_t len = ctrl >> 5;
            if (len == 7) { if (ip >= in_len) return false; len += in[ip++]; }
            if (ip >= in_len) return false;
            size_t dist = ((size_t)(ctrl & 31) << 8 | in[ip++]) + 1;
            len += 2;
            if (dist > op || op + len > out_len) return false;
            for (size_t k = 0; k < len; ++k, ++op) out[op] = out[op - dist];
        }
    }
    return op == out_len;
}

int pcd_load(const char* path, PcdHeader& h, std::vector<unsigned char>& aos) {
    File file(path, "rb"); FILE* f = file.f;
    if (!f) { set_error("%s: %s", path, strerror(errno)); return PCREG_E_ARG; }
    int rc = pcd_parse_header(f, h, path);               // leaves f at the payload, which the file's size backs
    if (rc) return rc;
    const size_t n = (size_t)h.points, ps = (size_t)h.point_size;
    aos.assign(n * ps, 0);
    if (h.data == PcdHeader::BINARY) {
        if (fread(aos.data(), 1, n * ps, f) != n * ps) { set_error("%s: truncated binary PCD", path); return PCREG_E_ARG; }
    } else if (h.data == PcdHeader::COMPRESSED) {
        uint32_t sz[2];
        if (fread(sz, 4, 2, f) != 2 || sz[1] != n * ps) { set_error("%s: bad binary_compressed sizes", path); return PCREG_E_ARG; }
        std::vector<unsigned char> in(sz[0]), soa(sz[1]);
        if (fread(in.data(), 1, sz[0], f) != sz[0] || !lzf_decompress(in.data(), sz[0], soa.data(), sz[1])) {
            set_error("%s: corrupt binary_compressed PCD", path); return PCREG_E_ARG;
        }
        size_t base = 0;                       // decompressed layout: field by field
        for (const PcdField& fd : h.fields) {
            const size_t w = (size_t)fd.size * fd.count;
            for (size_t i = 0; i < n; ++i) memcpy(&aos[i * ps + fd.offset], &soa[base + i * w], w);
            base += w * n;
        }
    } else {
        char tok[128];
        for (size_t i = 0; i < n; ++i)
            for (const PcdField& fd : h.fields)
                for (int c = 0; c < fd.count; ++c) {
                    if (fscanf(f, "%127s", tok) != 1) { set_error("%s: truncated ascii PCD (point %zu)", path, i); return PCREG_E_ARG; }
                    unsigned char* p = &aos[i * ps + fd.offset + (size_t)c * fd.size];
                    // the whole token has to be a number (nan and inf are): what is none is refused, not read as 0
                    char* end = nullptr; errno = 0;
                    const bool digit = tok[0] == '-' || tok[0] == '+' || (tok[0] >= '0' && tok[0] <= '9');
                    bool ok = strlen(tok) < 127;
                    if (fd.type == 'F') { if (fd.size == 4) { float v = strtof(tok, &end); memcpy(p, &v, 4); } else { double v = strtod(tok, &end); memcpy(p, &v, 8); } }
                    else if (fd.type == 'U') {             // no sign wrapped round, no value cut to the field's low bytes
                        unsigned long long v = strtoull(tok, &end, 10);
                        ok = ok && digit && tok[0] != '-' && errno == 0 && (fd.size == 8 || v >> (8 * fd.size) == 0);
                        memcpy(p, &v, fd.size);            // little-endian host
                    } else {
                        long long v = strtoll(tok, &end, 10);
                        const long long top = fd.size == 8 ? LLONG_MAX : (1LL << (8 * fd.size - 1)) - 1;
                        ok = ok && digit && errno == 0 && v <= top && v >= -top - 1;
                        memcpy(p, &v, fd.size);
                    }
                    if (!ok || end == tok || *end) { set_error("%s: ascii PCD: '%.40s' is no number its field holds (point %zu)", path, tok, i); return PCREG_E_ARG; }
                }
    }
    return PCREG_OK;
}

// ------------------------------------------------------------------------------------ MAT v5
enum { miINT8 = 1, miUINT8, miINT16, miUINT16, miINT32, miUINT32, miSINGLE, miDOUBLE = 9, miINT64 = 12, miUINT64, miMATRIX, miCOMPRESSED };
struct MatVar {
    std::string name; int cls = 0; std::vector<int> dims;
    bool numeric = false;                                // a real array of a numeric class: what this reader reads
    const char* bad = nullptr;                           // numeric, but not readable: why (said when it is the variable asked for)
    int rows = 0, cols = 0; int data_type = 0; const unsigned char* data = nullptr; size_t data_bytes = 0;
};

// one tag inside the `avail` bytes at p: its type, its byte count, where its payload starts (`hdr`) and how far the next element
// is (`step`, clamped to avail: a last element may come without its padding).  false = the tag or its payload is not all there
bool mat_read_tag(const unsigned char* p, size_t avail, uint32_t& type, uint32_t& bytes, size_t& hdr, size_t& step) {
    if (avail < 8) return false;
    uint32_t w0; memcpy(&w0, p, 4);
    if (w0 >> 16) { type = w0 & 0xFFFF; bytes = w0 >> 16; hdr = 4; step = 8; return bytes <= 4; }     // small element
    type = w0; memcpy(&bytes, p + 4, 4); hdr = 8;
    if (bytes > avail - 8) return false;
    step = std::min(avail, 8 + ((size_t)bytes + 7) / 8 * 8);
    return true;
}
size_t mat_type_size(int type) {                         // 0: not a numeric type
    switch (type) { case miDOUBLE: case miINT64: case miUINT64: return 8; case miSINGLE: case miINT32: case miUINT32: return 4;
                    case miINT16: case miUINT16: return 2; case miINT8: case miUINT8: return 1; default: return 0; }
}

// One miMATRIX body of n bytes, every read inside them.  A file is not refused for a variable that is merely passed on the way to
// another: true = the variable is listed -- a numeric one with its shape and data, or with the reason (`bad`) why it cannot be
// read; any other class (cell, struct, char, sparse, object, an opaque string / table / datetime object, which has no dimensions
// tag; a complex array) by its name alone, where it has one.  false = nothing to list.
bool mat_parse_matrix(const unsigned char* p, size_t n, MatVar& v) {
    size_t pos, h, step; uint32_t t, b;
    if (!mat_read_tag(p, n, t, b, h, step) || t != miUINT32 || b != 8 || h != 8) return false;   // no array flags
    uint32_t flags; memcpy(&flags, p + h, 4);
    v.cls = flags & 0xFF;
    v.numeric = v.cls >= 6 && v.cls <= 15 && !(flags & 0x0800);
    pos = step;
    bool have_dims = false, have_name = false;
    bool ok = mat_read_tag(p + pos, n - pos, t, b, h, step);
    if (ok && t == miINT32) {                            // dimensions (an opaque object goes straight on to its name)
        have_dims = b % 4 == 0;
        if (have_dims && b) { v.dims.resize(b / 4); memcpy(v.dims.data(), p + pos + h, b); }
        pos += step;
        ok = mat_read_tag(p + pos, n - pos, t, b, h, step);
    }
    if (ok && t == miINT8) { v.name.assign((const char*)p + pos + h, b); have_name = true; pos += step; }
    if (!v.numeric) return have_name;
    auto fault = [&]() -> const char* {
        if (!have_dims || v.dims.size() < 2) return "has no two or more dimensions";
        if (!have_name) return "has no name";
        if (!mat_read_tag(p + pos, n - pos, t, b, h, step)) return "has data that are not all there";
        if (!mat_type_size((int)t)) return "has data of no numeric type";
        // rows x cols with the trailing dimensions folded into cols: no negative, each and their product within int
        long r = v.dims[0], c = 1;
        if (r < 0) return "has a negative dimension";
        for (size_t k = 1; k < v.dims.size(); ++k) {
            if (v.dims[k] < 0) return "has a negative dimension";
            c *= v.dims[k];
            if (c > INT_MAX) return "has a shape beyond INT_MAX";
        }
        if (r * c > INT_MAX) return "has a shape beyond INT_MAX";
        if ((size_t)(r * c) * mat_type_size((int)t) > b) return "has fewer data than its shape";
        v.rows = (int)r; v.cols = (int)c;
        v.data_type = (int)t; v.data = p + pos + h; v.data_bytes = b;
        return nullptr;
    };
    v.bad = fault();
    return true;
}

int mat_load(const char* path, std::vector<std::vector<unsigned char>>& storage, std::vector<MatVar>& vars) {
    std::vector<unsigned char> file;
    {
        File in(path, "rb");
        if (!in.f) { set_error("%s: %s", path, strerror(errno)); return PCREG_E_ARG; }
        unsigned char buf[1 << 16]; size_t got;
        while ((got = fread(buf, 1, sizeof buf, in.f)) > 0) file.insert(file.end(), buf, buf + got);
    }
    if (file.size() < 128 || memcmp(file.data(), "MATLAB 5.0 MAT-file", 19) != 0) {
        set_error("%s: not a Level-5 MAT-file (v7.3 files are HDF5 and are not supported)", path); return PCREG_E_ARG;
    }
    if (file[126] != 'I' || file[127] != 'M') { set_error("%s: big-endian MAT-files are not supported", path); return PCREG_E_ARG; }
    // the bytes themselves stay where they are when `storage` grows (a moved vector keeps its block); its elements do not, so
    // the file is walked through a pointer to the bytes, not through a reference to storage.front()
    const unsigned char* const fl = file.data(); const size_t fl_size = file.size();
    storage.push_back(std::move(file));
    size_t pos = 128;
    while (pos + 8 <= fl_size) {
        uint32_t t, b; size_t h, step;
        if (!mat_read_tag(fl + pos, fl_size - pos, t, b, h, step)) { set_error("%s: truncated MAT-file", path); return PCREG_E_ARG; }
        const unsigned char* body = fl + pos + h;
        const char* bad = nullptr;
        if (t == miCOMPRESSED && h == 8) {
            // inflate with a growing buffer (the element holds exactly one miMATRIX)
            std::vector<unsigned char> out(std::max<size_t>(4 * (size_t)b, 1024));
            z_stream zs; memset(&zs, 0, sizeof zs);
            if (inflateInit(&zs) != Z_OK) { set_error("%s: zlib init failed", path); return PCREG_E_ARG; }
            zs.next_in = const_cast<unsigned char*>(body); zs.avail_in = b;
            size_t produced = 0; int zr;
            do {
                if (produced == out.size()) out.resize(out.size() * 2);
                zs.next_out = out.data() + produced; zs.avail_out = (uInt)std::min<size_t>(out.size() - produced, 1u << 30);
                zr = inflate(&zs, Z_NO_FLUSH);
                produced = zs.total_out;
            } while (zr == Z_OK);
            inflateEnd(&zs);
            if (zr != Z_STREAM_END) { set_error("%s: corrupt compressed element", path); return PCREG_E_ARG; }
            out.resize(produced);
            storage.push_back(std::move(out));
            const std::vector<unsigned char>& o = storage.back();
            uint32_t t2, b2; size_t h2, step2;
            if (!mat_read_tag(o.data(), o.size(), t2, b2, h2, step2) || t2 != miMATRIX || h2 != 8) bad = "a compressed element that does not hold a matrix";
            else if (b2) { MatVar v; if (mat_parse_matrix(o.data() + h2, b2, v)) vars.push_back(v); }
            step = 8 + (size_t)b;                        // compressed elements are not padded
        } else if (t == miMATRIX && h == 8 && b) {
            MatVar v; if (mat_parse_matrix(body, b, v)) vars.push_back(v);
        }
        if (bad) { set_error("%s: malformed MAT-file: %s", path, bad); return PCREG_E_ARG; }
        pos += step;
    }
    return PCREG_OK;
}

double mat_elem(const unsigned char* p, int type, size_t i) {
    switch (type) {
        case miDOUBLE: { double v; memcpy(&v, p + 8 * i, 8); return v; }
        case miSINGLE: { float v; memcpy(&v, p + 4 * i, 4); return v; }
        case miINT8: return ((const int8_t*)p)[i];   case miUINT8: return p[i];
        case miINT16: { int16_t v; memcpy(&v, p + 2 * i, 2); return v; }  case miUINT16: { uint16_t v; memcpy(&v, p + 2 * i, 2); return v; }
        case miINT32: { int32_t v; memcpy(&v, p + 4 * i, 4); return v; }  case miUINT32: { uint32_t v; memcpy(&v, p + 4 * i, 4); return v; }
        case miINT64: { int64_t v; memcpy(&v, p + 8 * i, 8); return (double)v; } case miUINT64: { uint64_t v; memcpy(&v, p + 8 * i, 8); return (double)v; }
        default: return NAN;
    }
}
// no exception leaves the C ABI: what a hostile file can provoke (std::bad_alloc, std::length_error) becomes PCREG_E_ARG
template <class F> int guarded(const char* path, F&& body) {
    try { return body(); }
    catch (const std::exception& e) { set_error("%s: %s", path ? path : "(null)", e.what()); return PCREG_E_ARG; }
    catch (...) { set_error("%s: unknown exception", path ? path : "(null)"); return PCREG_E_ARG; }
}

}  // namespace
}  // namespace pcreg

using namespace pcreg;

extern "C" {

int pcreg_pcd_info(const char* path, int* n_points, int* has_rgb) {
    PCREG_ARG(path && n_points);
    return guarded(path, [&]() -> int {
        File file(path, "rb");
        if (!file.f) { set_error("%s: %s", path, strerror(errno)); return PCREG_E_ARG; }
        PcdHeader h; int rc = pcd_parse_header(file.f, h, path);
        if (rc) return rc;
        *n_points = (int)h.points;                       // 0 .. INT_MAX, and the file is large enough to hold them
        if (has_rgb) *has_rgb = h.fc != nullptr;
        return PCREG_OK;
    });
}

int pcreg_pcd_read(const char* path, float* xyz, int ld, uint32_t* rgb, int n) {
    PCREG_ARG(path && xyz && n >= 0 && ld >= n);
    return guarded(path, [&]() -> int {
        PcdHeader h; std::vector<unsigned char> aos;
        int rc = pcd_load(path, h, aos);
        if (rc) return rc;
        if ((long)n != h.points) { set_error("%s holds %ld points, the buffer %d", path, h.points, n); return PCREG_E_ARG; }
        for (int i = 0; i < n; ++i) {
            const unsigned char* p = &aos[(size_t)i * h.point_size];
            xyz[i] = pcd_value(p + h.fx->offset, *h.fx); xyz[i + (size_t)ld] = pcd_value(p + h.fy->offset, *h.fy);
            xyz[i + 2 * (size_t)ld] = pcd_value(p + h.fz->offset, *h.fz);
            if (rgb) { uint32_t c = 0; if (h.fc) memcpy(&c, p + h.fc->offset, 4); rgb[i] = c; }   // packed 0x00RRGGBB, whatever TYPE says; the field is 4 bytes
        }
        return PCREG_OK;
    });
}

int pcreg_pcd_write(const char* path, const float* xyz, int n, int ld, const uint32_t* rgb, int binary) {
    PCREG_ARG(path && xyz && n >= 0 && ld >= n);
    return guarded(path, [&]() -> int {
        File file(path, "wb"); FILE* f = file.f;
        if (!f) { set_error("%s: %s", path, strerror(errno)); return PCREG_E_ARG; }
        fprintf(f, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\n");
        if (rgb) fprintf(f, "FIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n");
        else     fprintf(f, "FIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n");
        fprintf(f, "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n", n, n, binary ? "binary" : "ascii");
        for (int i = 0; i < n; ++i) {
            const float p[3] = {xyz[i], xyz[i + (size_t)ld], xyz[i + 2 * (size_t)ld]};
            if (binary) { fwrite(p, 4, 3, f); if (rgb) fwrite(&rgb[i], 4, 1, f); }
            else if (rgb) fprintf(f, "%.9g %.9g %.9g %u\n", p[0], p[1], p[2], rgb[i]);
            else fprintf(f, "%.9g %.9g %.9g\n", p[0], p[1], p[2]);
        }
        file.f = nullptr;                                // closed here, for its result
        if (fclose(f) != 0) { set_error("%s: write failed", path); return PCREG_E_ARG; }
        return PCREG_OK;
    });
}

// Variable `name` (NULL or "" = the first numeric array) of a Level-5 MAT-file: rows x cols (further
// dimensions folded into cols).  With out == NULL only the shape is returned.
int pcreg_mat_read_double(const char* path, const char* name, double* out, int* rows, int* cols) {
    PCREG_ARG(path && rows && cols);
    return guarded(path, [&]() -> int {
        std::vector<std::vector<unsigned char>> storage; storage.reserve(64);
        std::vector<MatVar> vars;
        int rc = mat_load(path, storage, vars);
        if (rc) return rc;
        const MatVar* v = nullptr;
        for (const MatVar& c : vars) {
            if (name && *name) { if (c.name == name) { v = &c; break; } }
            else if (c.numeric) { v = &c; break; }
        }
        if (!v) { set_error("%s: no variable '%s'", path, name && *name ? name : "<first numeric>"); return PCREG_E_ARG; }
        if (!v->numeric) { set_error("%s: variable '%s' is not a real numeric array", path, v->name.c_str()); return PCREG_E_ARG; }
        if (v->bad) { set_error("%s: variable '%s' %s", path, v->name.c_str(), v->bad); return PCREG_E_ARG; }
        *rows = v->rows; *cols = v->cols;                // validated by mat_parse_matrix: non-negative, the product within int and within the data
        const size_t count = (size_t)v->rows * v->cols;
        if (out) for (size_t i = 0; i < count; ++i) out[i] = mat_elem(v->data, v->data_type, i);
        return PCREG_OK;
    });
}

}  // extern "C"
