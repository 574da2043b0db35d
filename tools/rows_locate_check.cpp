// Host check of the batch search k_unique_rows runs per wave (kary_last_le, rows_window_batch: hkv_batch_dev.h)
// against batch_of's binary search, over random and adversarial offset arrays. A block is emulated as the kernel
// runs it: narrow to a window for the block's first position, then every position reads its batch from the
// window, or reports that the window ended first (the kernel then asks batch_of). Built with the host compiler
// under -fsanitize=address,undefined and run by tests/test_rows_locate_host.py; prints "rows locate: OK".
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "hkv_batch_dev.h"

using hkv::kRowsWindow;

static long g_checked = 0, g_fallbacks = 0, g_steps_max = 0;

// batch_of's packed branch: the last batch whose offset is <= i
static int32_t ref_batch(const std::vector<int32_t> &off, int32_t n, int64_t i)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

static bool fail(const char *what, const char *name, int32_t n, int64_t i, long got, long want)
{
    std::printf("FAIL %s: %s n_batches %d position %lld got %ld want %ld\n", name, what, n, (long long)i, got, want);
    return false;
}

// off: n + 1 offsets. Every block of E positions (or `blocks` of them, spread over the launch) is checked.
static bool check(const char *name, const std::vector<int32_t> &off, int E, long blocks = 0)
{
    const int32_t n = (int32_t)off.size() - 1;
    const int64_t n_live = off[n];
    const int64_t nblk = (n_live + E - 1) / E;
    const int64_t stride = blocks && nblk > blocks ? nblk / blocks : 1;
    for (int64_t blk = 0; blk < nblk; blk += stride) {
        const int64_t i0 = blk * E;
        long steps = 0;
        const auto count = [&](int32_t lo, int32_t hi) {
            int32_t c = 0;
            bool open = true;   // the samples at or below hi that are <= i0 are a prefix
            for (int s = 0; s < 64; ++s) {
                const int32_t idx = hkv::kary_sample(lo, hi, s);
                const bool in = idx <= hi && off[idx] <= i0;   // reads no offset past hi
                if (in && !open) return -1000;
                if (in) ++c; else open = false;
            }
            ++steps;
            return c;
        };
        const int32_t whole = hkv::kary_last_le(n, 0, count);
        if (whole != ref_batch(off, n, i0)) return fail("whole search", name, n, i0, whole, ref_batch(off, n, i0));
        steps = 0;
        const int32_t lo = hkv::kary_last_le(n, kRowsWindow / 2 - 1, count);
        if (steps > g_steps_max) g_steps_max = steps;
        if (n <= (1 << 18) && steps > 2) return fail("narrowing steps", name, n, i0, steps, 2);
        const auto win = [&](int32_t k) {
            if (k < 0 || k >= kRowsWindow) std::abort();
            return lo + k < n ? off[lo + k] : INT32_MAX;
        };
        int32_t k0 = -1;
        for (int k = 0; k < 64; ++k) k0 += win(k) <= i0;
        if (k0 < 0) k0 = 0;
        if (lo + k0 != ref_batch(off, n, i0)) return fail("block's first batch", name, n, i0, lo + k0, ref_batch(off, n, i0));
        for (int t = 0; t < E && i0 + t < n_live; ++t) {
            const int64_t i = i0 + t;
            int32_t b = -1;
            const bool in = hkv::rows_window_batch(win, lo, k0, i, i0 + E - 1, b);
            const int32_t want = ref_batch(off, n, i);
            ++g_checked;
            if (in) {
                if (b != want) return fail("window batch", name, n, i, b, want);
            } else {
                ++g_fallbacks;
                if (want < lo + kRowsWindow - 1) return fail("fallback inside the window", name, n, i, want, lo);
            }
        }
    }
    return true;
}

static std::vector<int32_t> from_counts(const std::vector<int32_t> &cnt)
{
    std::vector<int32_t> off(cnt.size() + 1, 0);
    for (size_t b = 0; b < cnt.size(); ++b) off[b + 1] = off[b] + cnt[b];
    return off;
}

int main()
{
    std::mt19937_64 rng(20240607);
    bool ok = true;
    for (int E : {32, 64}) {
        // one batch; one element in all
        ok = ok && check("one batch", from_counts({200}), E);
        ok = ok && check("one element", from_counts({1}), E);
        // all batches empty but one: the first, the last, one in the middle
        for (int32_t n : {2, 63, 64, 65, 129, 4097, 100003}) {
            for (int32_t at : {0, n / 2, n - 1}) {
                std::vector<int32_t> c(n, 0);
                c[at] = 777;
                ok = ok && check("all empty but one", from_counts(c), E);
            }
        }
        // runs of more than a window of empty batches between busy ones; first and last batch empty
        for (int32_t run : {kRowsWindow - 2, kRowsWindow - 1, kRowsWindow, kRowsWindow + 1, 3 * kRowsWindow, 5000}) {
            std::vector<int32_t> c;
            c.push_back(0);
            for (int rep = 0; rep < 4; ++rep) {
                for (int j = 0; j < 5; ++j) c.push_back(1 + (int32_t)(rng() % 40));
                for (int j = 0; j < run; ++j) c.push_back(0);
            }
            c.push_back(9);
            c.push_back(0);
            const long before = g_fallbacks;
            ok = ok && check("runs of empty batches", from_counts(c), E);
            if (ok && run > kRowsWindow && g_fallbacks == before) ok = fail("no fallback after a long run", "runs", run, 0, 0, 1);
        }
        // every batch one element: offsets equal to i, i - 1 and i + 1 around every position; and two, and E +- 1
        for (int32_t per : {1, 2, E - 1, E, E + 1, 3 * E + 1}) {
            for (int32_t n : {1, 3, 64, 65, 4096, 4097, 20001}) {
                ok = ok && check("equal batches", from_counts(std::vector<int32_t>(n, per)), E);
            }
        }
        // random ragged batches, n_batches not a power of two, up to 2^18
        for (int32_t n : {5, 100, 1000, 16384, 65537, 200003, (1 << 18) - 1, 1 << 18}) {
            for (int mean : {0, 3, 16}) {
                std::vector<int32_t> c(n);
                for (auto &x : c) x = mean == 0 ? (rng() % 16 == 0 ? (int32_t)(rng() % 50) : 0) : (int32_t)(rng() % (2 * mean + 1));
                ok = ok && check("random", from_counts(c), E, 20000);
            }
        }
    }
    // past 2^18 batches the narrowing takes a third step and the answers are the same
    {
        std::vector<int32_t> c((1 << 20) + 77);
        for (auto &x : c) x = (int32_t)(rng() % 3);
        ok = ok && check("2^20 batches", from_counts(c), 64, 5000);
        if (ok && g_steps_max != 3) ok = fail("steps past 2^18 batches", "2^20", 1 << 20, 0, g_steps_max, 3);
    }
    if (!ok) return 1;
    std::printf("rows locate: OK (%ld positions, %ld past their window)\n", g_checked, g_fallbacks);
    return 0;
}
