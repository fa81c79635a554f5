// Probe: is the transposing row reduction of the conv statistics tails
// (row_stats16, common.h -- the function the kernels call) bitwise
// row_sum16's lane-0 result, and does exactly one lane park each total in its
// own slot?  Every row of every wave gets partials s1[J][4] / s2[J][4] per
// lane -- random, mixed magnitudes, cancelling lane pairs, denormals, exact
// integers -- for J = 1, 2, 3, 4 (8, 16, 16 + 8 and 32 values a round), as
// doubles and as floats (the streaming kernels' partials, widened on arrival);
// prints the number of differing bits and of slots not parked exactly once
// per (type, J) (all must be 0) and exits non-zero otherwise.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include \
//     -I../../dl-normalizing-flows_amd/csrc row_reduce_check.hip -o row_reduce_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.h"

// in: [rows][16 lanes][8 J] (order (j * 4 + r) * 2 + which); ref / got: [rows][8 J]; parks: [rows][8 J]
template <typename F, int J>
__global__ void k_check(const F* in, double* ref, double* got, int* parks, int rows) {
    constexpr int N = 8 * J;
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 4, li = threadIdx.x & 15;
    const int rr = row < rows ? row : 0;   // (every lane of a row stays active; a surplus row writes nothing)
    const bool live = row < rows;
    F s1[J][4], s2[J][4];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s1[j][r] = in[((long long)rr * 16 + li) * N + (j * 4 + r) * 2];
            s2[j][r] = in[((long long)rr * 16 + li) * N + (j * 4 + r) * 2 + 1];
        }
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double t1 = row_sum16((double)s1[j][r]), t2 = row_sum16((double)s2[j][r]);
            if (li == 0 && live) {
                ref[(long long)rr * N + (j * 4 + r) * 2] = t1;
                ref[(long long)rr * N + (j * 4 + r) * 2 + 1] = t2;
            }
        }
    row_stats16(s1, s2, li, [&](int j, int r, int which, double u) {
        if (!live || j < 0 || j >= J || r < 0 || r >= 4 || which < 0 || which > 1) return;
        const long long o = (long long)rr * N + (j * 4 + r) * 2 + which;
        got[o] = u;
        atomicAdd(&parks[o], 1);
    });
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }
static double from_bits(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// one row's 16 x n inputs of a given kind (values a float holds too where flt)
static void fill(double* p, int n, int kind, bool flt) {
    const int span = flt ? 60 : 600;
    for (int i = 0; i < 16 * n; ++i) {
        switch (kind) {
        case 0: p[i] = uni(); break;                                                   // random
        case 1: p[i] = uni() * ldexp(1.0, (int)(rnd() % span) - span / 2); break;   // mixed magnitudes
        case 2: {   // cancellation: lane li ^ bit holds nearly the negative (bit = the pair distance, by input)
            const int li = i / n, bit = 1 << ((i % n) & 3);
            const double eps = flt ? 0x1p-23 : 0x1p-52;
            p[i] = (li & bit) ? -p[i - bit * n] * (1.0 + (double)(rnd() % 3) * eps) : uni() * 1e10;
            break;
        }
        case 3: p[i] = flt ? ldexp(uni(), -140) : from_bits(rnd() & 0x800fffffffffffffull); break;   // denormals
        case 4: p[i] = (rnd() % 4) ? (flt ? ldexp(uni(), -135) : from_bits(rnd() & 0x800fffffffffffffull))
                                   : uni() * (flt ? 0x1p-120 : 0x1p-1020); break;
        case 5: p[i] = (double)((long long)(rnd() % 33554432) - 16777216); break;     // exact integers
        default: p[i] = (rnd() % 8 == 0) ? uni() * 1e16 : uni(); break;               // a few large among small
        }
    }
}

template <typename F, int J>
static long long run(int rows) {
    constexpr int N = 8 * J;
    constexpr bool flt = std::is_same<F, float>::value;
    std::vector<double> ind((size_t)rows * 16 * N);
    for (int r = 0; r < rows; ++r) fill(&ind[(size_t)r * 16 * N], N, r % 7, flt);
    std::vector<F> in(ind.size());
    for (size_t i = 0; i < in.size(); ++i) in[i] = (F)ind[i];
    F* din;
    double *dref, *dgot;
    int* dparks;
    const size_t nout = (size_t)rows * N;
    hipMalloc(&din, in.size() * sizeof(F));
    hipMalloc(&dref, nout * 8);
    hipMalloc(&dgot, nout * 8);
    hipMalloc(&dparks, nout * 4);
    hipMemcpy(din, in.data(), in.size() * sizeof(F), hipMemcpyHostToDevice);
    hipMemset(dref, 0xff, nout * 8);
    hipMemset(dgot, 0xee, nout * 8);
    hipMemset(dparks, 0, nout * 4);
    const int threads = rows * 16;
    k_check<F, J><<<(threads + 255) / 256, 256>>>(din, dref, dgot, dparks, rows);
    if (hipDeviceSynchronize() != hipSuccess) {
        printf("%s J = %d: launch failed\n", flt ? "fp32" : "fp64", J);
        return -1;
    }
    std::vector<uint64_t> ref(nout), got(nout);
    std::vector<int> parks(nout);
    hipMemcpy(ref.data(), dref, nout * 8, hipMemcpyDeviceToHost);
    hipMemcpy(got.data(), dgot, nout * 8, hipMemcpyDeviceToHost);
    hipMemcpy(parks.data(), dparks, nout * 4, hipMemcpyDeviceToHost);
    long long bits = 0, nonzero = 0, badpark = 0;
    for (size_t i = 0; i < nout; ++i) {
        nonzero += (ref[i] << 1) != 0;
        bits += __builtin_popcountll(ref[i] ^ got[i]);
        badpark += parks[i] != 1;
    }
    printf("%s J = %d (%2d values per lane): %d rows, %zu sums (%lld non-zero), differing bits %lld, slots not parked once %lld\n",
           flt ? "fp32" : "fp64", J, N, rows, nout, nonzero, bits, badpark);
    hipFree(din);
    hipFree(dref);
    hipFree(dgot);
    hipFree(dparks);
    return bits + badpark;
}

int main() {
    const int rows = 7 * 600 + 3;   // a partial last workgroup
    long long bad = 0;
    bad |= run<double, 1>(rows);
    bad |= run<double, 2>(rows);
    bad |= run<double, 3>(rows);
    bad |= run<double, 4>(rows);
    bad |= run<float, 1>(rows);
    bad |= run<float, 2>(rows);
    bad |= run<float, 3>(rows);
    bad |= run<float, 4>(rows);
    printf(bad ? "FAIL\n" : "OK: every sum bitwise row_sum16's lane 0, parked once by its own lane\n");
    return bad ? 1 : 0;
}
