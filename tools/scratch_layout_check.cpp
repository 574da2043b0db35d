// The batch scratch layout against the figures it had when batch_scratch_bytes and batch_carve each wrote it out:
// the size by that formula, every carved array at its offset. Host only; links libhermeskv.so.
//   hipcc -std=c++17 -I hermes_amd/csrc tools/scratch_layout_check.cpp -L hermes_amd -lhermeskv -o scratch_layout_check
#include <cstdio>

#include "hkv_internal.h"

static size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

int main()
{
    int bad = 0;
    const int64_t caps[] = {1, 250, 2048, 1 << 20};
    const uint32_t sizes[] = {64, 320};
    for (int64_t cap : caps)
        for (uint32_t es : sizes) {
            const size_t c = (size_t)cap;
            const size_t want = a256(4 * c) * 3 + a256(c) + a256(16 * c) * 2 + 256 + a256(2 * c) + a256((size_t)es * c);
            const size_t got = hkv::batch_scratch_bytes(cap, es);
            alignas(256) static uint8_t base[256];   // only its address is used
            hkv::BatchLaunch bl{};
            hkv::batch_carve(bl, base, cap, es);
            const struct {
                const char *name;
                const void *p;
                size_t bytes;
            } arr[] = {{"ent", bl.ent, 4 * c},    {"st", bl.st, c},           {"mem", bl.mem, 16 * c},
                       {"fbl", bl.fbl, 4 * c},    {"pf", bl.pf, 4 * c},       {"shadow", bl.shadow, (size_t)es * c},
                       {"ctr", bl.ctr, 256},      {"hx", bl.hx, 16 * c},      {"fk", bl.fk, 2 * c}};
            size_t off = 0;
            for (const auto &x : arr) {
                if ((const uint8_t *)x.p != base + off) {
                    printf("cap %lld entry %u: %s at %td, expected %zu\n", (long long)cap, es, x.name,
                           (const uint8_t *)x.p - base, off);
                    ++bad;
                }
                off += a256(x.bytes);
            }
            if (got != want || off != want || bl.cap != (uint32_t)cap) {
                printf("cap %lld entry %u: size %zu, carved %zu, expected %zu (cap member %u)\n", (long long)cap, es, got,
                       off, want, bl.cap);
                ++bad;
            }
        }
    printf("%s\n", bad ? "FAILED" : "scratch layout: OK");
    return bad != 0;
}
