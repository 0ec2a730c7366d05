// TEST INFRASTRUCTURE ONLY -- the raw-array files the shim drivers exchange with their tests: a file is the array's bytes, nothing else.
#ifndef SHIM_DRIVER_IO_HPP
#define SHIM_DRIVER_IO_HPP
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

template <class T> std::vector<T> load(const std::string& path)
{
    std::vector<T> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T));
    if (n && fread(v.data(), sizeof(T), v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
template <class T> void dump(const std::string& path, const T* p, size_t n)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (n) fwrite(p, sizeof(T), n, f);
    fclose(f);
}
template <class T> void dump(const std::string& path, const std::vector<T>& v) { dump(path, v.data(), v.size()); }
#endif
