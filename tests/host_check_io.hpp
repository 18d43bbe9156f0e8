// The files of the stand-alone CPU checks (tests/host_*_check.cpp): a whole file as bytes, bytes as records, a checked write.
#ifndef SUSHI_HOST_CHECK_IO_HPP
#define SUSHI_HOST_CHECK_IO_HPP

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace host_check {

// the file's bytes; exits with 2 if it cannot be opened
inline std::vector<unsigned char> read_file(const char* path) {
    std::vector<unsigned char> buf;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    unsigned char tmp[65536];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    std::fclose(f);
    return buf;
}

// the whole records of type T that `bytes` holds (bytes behind the last one are ignored)
template <class T>
std::vector<T> records(const std::vector<unsigned char>& bytes) {
    std::vector<T> v(bytes.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), bytes.data(), v.size() * sizeof(T));
    return v;
}

// Arrays written back to back into a new file; the program's exit status: 0, or 2 if the file could not be opened or a write
// fell short.
struct Part { const void* data; size_t bytes; };
template <class T>
Part part(const std::vector<T>& v) { return Part{v.data(), v.size() * sizeof(T)}; }
inline int write_file(const char* path, std::initializer_list<Part> parts) {
    FILE* f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot write %s\n", path); return 2; }
    bool ok = true;
    for (const Part& p : parts) ok = ok && (p.bytes == 0 || std::fwrite(p.data, 1, p.bytes, f) == p.bytes);
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

}  // namespace host_check
#endif
