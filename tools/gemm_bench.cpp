// Standalone timing harness for csrc/gemm.hip at the cfg-B shapes of the step (links build/exp/gemm.o directly; the object goes in front of the source, which hipcc compiles as HIP):
//   make -C few-shot-music-generation_amd/csrc experiments && hipcc --offload-arch=gfx950 -O3 -std=c++17 \
//       -Ifew-shot-music-generation_amd/csrc -Iinclude few-shot-music-generation_amd/build/exp/gemm.o tools/gemm_bench.cpp -o tools/gemm_bench.bin   (make -C few-shot-music-generation_amd/csrc experiments: the stamped instantiations live in the experiment build)
// Usage: gemm_bench.bin [reps] [blocks_per_cu] [verify 0/1: compare every result with a naive fp32 kernel]      (blocks_per_cu < 4 applies the aux-stream LDS cap)
// Prints per shape: ksplit, kernel-only ms (GEMM without the slab reduce), total ms, TF on the total.
// EPI=0 (default) plain store without bias; EPI=1 plain store with bias (the x-part GEMM's epilogue); EPI=2 forward-only cross entropy;
// EPI=3 fused-softmax store (the train step's projection) -- bias, ce_part, ce_tgt, ce_nvocab, ce_store filled as api_forward.hip does.
// 2 and 3 apply where the step uses them (<KC,XC>, unsplit K; 3: BX3 != 0); other shapes keep the plain store.  verify checks EPI <= 1.
#include "fsmg_kernels.h"
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <vector>
using namespace fsmg;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

struct Shape { const char* name; int amode, bmode; int M, N, K; int ksplit; bool colsum; };

// reference: one thread per element, fp64 accumulation
__global__ void k_ref(const float* A, int lda, int amode, const float* B, int ldb, int bmode, float* C, int M, int N, int K, const float* bias) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)M * N) return;
    const int m = (int)(i / N), n = (int)(i % N);
    double s = 0.0;                 // exact products, fp64 sum: what every kernel's error is measured against
    for (int k = 0; k < K; ++k) {
        const float a = (amode == OP_KC) ? A[(long long)m * lda + k] : A[(long long)k * lda + m];
        const float b = (bmode == OP_KC) ? B[(long long)n * ldb + k] : B[(long long)k * ldb + n];
        s += (double)a * (double)b;
    }
    C[i] = (float)(s + (bias ? (double)bias[n] : 0.0));
}
__global__ void k_ref_colsum(const float* B, int ldb, float* cs, int N, int K) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += B[(long long)k * ldb + n];
    cs[n] = (float)s;
}
static double rms_rel(const float* d_a, const float* d_b, size_t n) {
    std::vector<float> a(n), b(n);
    CK(hipMemcpy(a.data(), d_a, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), d_b, n * 4, hipMemcpyDeviceToHost));
    double e = 0, r = 0;
    for (size_t i = 0; i < n; ++i) { double d = (double)a[i] - b[i]; e += d * d; r += (double)b[i] * b[i]; }
    return std::sqrt(e / (r > 0 ? r : 1));
}
static double max_rel(const float* d_a, const float* d_b, size_t n) {
    std::vector<float> a(n), b(n);
    CK(hipMemcpy(a.data(), d_a, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), d_b, n * 4, hipMemcpyDeviceToHost));
    double e = 0, r = 0;
    for (size_t i = 0; i < n; ++i) { double d = std::fabs((double)a[i] - b[i]); if (!(d <= e)) e = d; r = std::max(r, (double)std::fabs(b[i])); }
    return e / (r > 0 ? r : 1);
}

// DIST=0 (default): uniform on [-0.5, 0.5).  DIST=1: sign * mantissa * 2^e with e uniform on [-30, 30] (sixty binades in
// one operand: the split must be exact at every magnitude).  DIST=2: 1e4 * uniform -- products of 1e8 that cancel to sums of
// O(1e8 sqrt K): errors are reported relative to max|C|, so this checks that no piece is dropped at large magnitudes.
static float* dev_random(size_t n, unsigned seed) {
    static const int dist = getenv("DIST") ? atoi(getenv("DIST")) : 0;
    std::vector<float> h(n);
    unsigned s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        float u = ((s >> 8) & 0xffff) / 65536.0f - 0.5f;
        if (dist == 1) { s = s * 1664525u + 1013904223u; u = std::ldexp(u + (u < 0 ? -0.5f : 0.5f), (int)((s >> 10) % 61) - 30); }
        else if (dist == 2) u *= 1e4f;
        h[i] = u;
    }
    float* d; CK(hipMalloc(&d, n * 4)); CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
}

// PROF=1 (with BX3=1): one more launch of the shape through the stamped instantiation of k_gemm_bx3; prints where a wave's
// cycles go per k tile, the prologue / epilogue share of a block's life and how many blocks a CU had in their k loop over time
static void profile_launch(hipStream_t s, int amode, int bmode, GemmArgs g, int pad, int blocks, float ms_plain) {
    const int NW = g.bx3 >= 2 ? 8 : 4;                  // waves per block (bx3 == 2: 4 multipliers + 4 loaders; 3: 8 of 128 x 64)
    unsigned long long* d; const size_t n = (size_t)blocks * NW * 8;
    CK(hipMalloc(&d, n * 8)); CK(hipMemset(d, 0, n * 8));
    g.prof = d;
    g.dbg = getenv("DBG") ? atoi(getenv("DBG")) : 0;
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    CK(launch_gemm(s, amode, bmode, g, pad));             // warm the instantiation
    CK(hipEventRecord(a, s)); for (int i = 0; i < 10; ++i) CK(launch_gemm(s, amode, bmode, g, pad)); CK(hipEventRecord(b, s)); CK(hipEventSynchronize(b));
    float ms; CK(hipEventElapsedTime(&ms, a, b)); ms /= 10;     // (the stamps kept are the last launch's)
    std::vector<unsigned long long> h(n);
    CK(hipMemcpy(h.data(), d, n * 8, hipMemcpyDeviceToHost));
    const int per = g.ksplit > 1 ? ((g.K + g.ksplit - 1) / g.ksplit + 15) / 16 * 16 : g.K;
    const double nk = (per + 15) / 16;
    // s_memtime is per XCD: normalise every stamp by the earliest entry seen on its XCD
    unsigned long long base[16]; for (auto& v : base) v = ~0ull;
    for (size_t w = 0; w < (size_t)blocks * NW; ++w) { const unsigned long long* o = &h[w * 8]; if (o[6]) { auto& m = base[(o[7] >> 32) & 15]; m = std::min(m, o[0]); } }
    double span = 0;
    for (int role = 0; role < (g.bx3 == 2 ? 2 : 1); ++role) {
        double mf = 0, cm = 0, bar = 0, pro = 0, epi = 0, life = 0, loop = 0; size_t cnt = 0;
        for (size_t w = 0; w < (size_t)blocks * NW; ++w) {
            if (g.bx3 == 2 && (int)((w % NW) >= (size_t)(NW / 2)) != role) continue;
            const unsigned long long* o = &h[w * 8];
            if (o[6] == 0) continue;
            mf += o[2]; cm += o[3]; bar += o[4]; pro += o[1] - o[0]; epi += o[6] - o[5]; life += o[6] - o[0]; loop += o[5] - o[1]; ++cnt;
            span = std::max(span, (double)(o[6] - base[(o[7] >> 32) & 15]));
        }
        printf("    PROF %s: per wave and k tile (ticks): reads+MFMA issue %.0f  loads wait+split+LDS write %.0f  drain+barrier %.0f  (sum %.0f) | per block: prologue %.0f  loop %.0f  epilogue %.0f  -> pro+epi %.1f %% of its life\n",
               g.bx3 == 2 ? (role ? "loaders    " : "multipliers") : "", mf / cnt / nk, cm / cnt / nk, bar / cnt / nk, (mf + cm + bar) / cnt / nk, pro / cnt, loop / cnt, epi / cnt, 100.0 * (pro + epi) / life);
    }
    printf("    PROF: stamped launch %.3f ms (plain %.3f); span %.0f ticks -> %.0f MHz; %.0f k tiles per block; MFMA pipe floor 768 ticks per k tile and wave\n", ms, ms_plain, span, span / (ms * 1e3), nk);
    // blocks resident / in their k loop per CU over time (wave 0 of every block)
    struct Iv { double a, b, c, e; unsigned key; };
    std::vector<Iv> iv;
    for (int bl = 0; bl < blocks; ++bl) {
        const unsigned long long* o = &h[(size_t)bl * NW * 8];
        if (o[6] == 0) continue;
        const unsigned long long bs = base[(o[7] >> 32) & 15];
        iv.push_back({(double)(o[0] - bs), (double)(o[1] - bs), (double)(o[5] - bs), (double)(o[6] - bs), (unsigned)((o[7] >> 32) & 0xf) << 8 | (unsigned)((o[7] >> 8) & 0xff)});
    }
    std::vector<unsigned> keys; for (auto& v : iv) keys.push_back(v.key);
    std::sort(keys.begin(), keys.end()); keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int NB = 16;
    double inloop[NB] = {0}, resident[NB] = {0};
    for (auto& v : iv) for (int q = 0; q < NB; ++q) {
        const double lo = span * q / NB, hi = span * (q + 1) / NB;
        resident[q] += std::max(0.0, std::min(hi, v.e) - std::max(lo, v.a)) / (hi - lo);
        inloop[q] += std::max(0.0, std::min(hi, v.c) - std::max(lo, v.b)) / (hi - lo);
    }
    printf("    PROF: %zu CUs seen; blocks per CU resident / in their k loop over %d time bins: ", keys.size(), NB);
    double tot_r = 0, tot_l = 0;
    for (int q = 0; q < NB; ++q) { printf("%.2f/%.2f ", resident[q] / keys.size(), inloop[q] / keys.size()); tot_r += resident[q]; tot_l += inloop[q]; }
    printf("| mean %.2f / %.2f\n", tot_r / NB / keys.size(), tot_l / NB / keys.size());
    CK(hipFree(d));
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 20;
    const int bpc = argc > 2 ? atoi(argv[2]) : 4;
    const int pad = gemm_lds_pad_for(bpc);
    const bool verify = argc > 3 && atoi(argv[3]) != 0;
    const int TB = 5760, H = 512, V = 10004, E = 256;
    Shape shapes[] = {
        {"logits  Hout*W      <KC,XC>", OP_KC, OP_XC, TB, V, H, 1, false},
        {"dhout   dlogits*W^T <KC,KC>", OP_KC, OP_KC, TB, H, V, 0, false},
        {"dW      Hout^T*dlog <XC,XC>", OP_XC, OP_XC, H, V, TB, 0, true},
        {"dW      (no colsum) <XC,XC>", OP_XC, OP_XC, H, V, TB, 0, false},
        {"dKh     Hprev^T*dZ  <XC,XC>", OP_XC, OP_XC, H, 4 * H, TB, 0, true},
        {"zx      X*Kx        <KC,XC>", OP_KC, OP_XC, TB, 4 * H, E, 1, false},
        // the two weight gradients with the activations handed over TRANSPOSED (k = rows contiguous): 16-byte loads for A
        {"dWt     HoutT*dlog  <KC,XC>", OP_KC, OP_XC, H, V, TB, 0, true},
        {"dKht    HprevT*dZ   <KC,XC>", OP_KC, OP_XC, H, 4 * H, TB, 0, true},
        // one of the 8 time chunks of the two-stream schedule (16 steps x 45 sequences)
        {"logits/8 chunk      <KC,XC>", OP_KC, OP_XC, TB / 8, V, H, 1, false},
        {"dhout/8  chunk      <KC,KC>", OP_KC, OP_KC, TB / 8, H, V, 0, false},
        // edge shapes (partial M/N tiles, K not a multiple of 16, K < 16)
        {"edge    <KC,XC> 70x52x20   ", OP_KC, OP_XC, 70, 52, 20, 1, false},
        {"edge    <KC,KC> 130x48x44  ", OP_KC, OP_KC, 130, 48, 44, 0, false},
        {"edge    <XC,XC> 48x260x49  ", OP_XC, OP_XC, 48, 260, 49, 0, true},
        {"edge    <XC,XC> 16x64x7    ", OP_XC, OP_XC, 16, 64, 7, 1, true},
        {"edge    <KC,XC> 6x200x12   ", OP_KC, OP_XC, 6, 200, 12, 1, false},
        // 256 block tiles that are all edge tiles of the 256 x 256-tile kernel (BX3=3): 128 live rows each (waves 4-7 multiply nothing) /
        // 20 live columns each (cfg-B's last column tile: two live sub-tiles, remapped onto two SIMDs)
        {"halfrow <KC,XC> 128x65536x512", OP_KC, OP_XC, 128, 65536, 512, 1, false},
        {"sliver  <KC,XC> 65536x20x512 ", OP_KC, OP_XC, 65536, 20, 512, 1, false},
    };
    hipStream_t s; CK(hipStreamCreate(&s));
    hipEvent_t e0, e1, e2; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); CK(hipEventCreate(&e2));
    float* slabs; CK(hipMalloc(&slabs, (size_t)16 * 5760 * 512 * 4 + (size_t)16 * 512 * 10004 * 4));
    float* csl; CK(hipMalloc(&csl, 32 * 10004 * 4));
    // XCD_FIRST=k: every GEMM as a work-queue launch restricted to the XCDs >= k (GemmArgs::xcd_first) + its clean-up launch;
    // XCD_FIRST=-1: the clean-up (chip-wide work-queue) launch alone
    const int xcd_first = getenv("XCD_FIRST") ? atoi(getenv("XCD_FIRST")) : 0;
    const int bx3 = getenv("BX3") ? atoi(getenv("BX3")) : 0;      // BX3=1: the bf16-split kernel (k_gemm_bx3)
    int* ctl; CK(hipMalloc(&ctl, 4 * 65536));
    const char* only = getenv("ONLY");                         // ONLY=substring of the shape name
    const int epi = getenv("EPI") ? atoi(getenv("EPI")) : 0;
    for (const Shape& sh : shapes) {
        if (only && !strstr(sh.name, only)) continue;
        const size_t an = (size_t)sh.M * sh.K, bn = (size_t)sh.K * sh.N, cn = (size_t)sh.M * sh.N;
        float* A = dev_random(an, 1); float* B = dev_random(bn, 2);
        float* C; CK(hipMalloc(&C, cn * 4)); float* cs; CK(hipMalloc(&cs, sh.N * 4));
        float* Cref = nullptr; float* csref = nullptr;
        // the epilogue's inputs (EPI=): a bias per column, and for the cross-entropy modes one (max, sum) slot per row and 64-column
        // slice, a target id per row and the target logits
        const bool ce = epi >= 2 && sh.amode == OP_KC && sh.bmode == OP_XC && sh.ksplit == 1 && (epi == 2 || bx3 != 0);
        const int nparts = 2 * ((sh.N + 127) / 128), nvocab = std::max(1, sh.N - 3);
        float* bias = epi >= 1 ? dev_random((size_t)sh.N, 3) : nullptr;
        float2* ce_part = nullptr; int* ce_tgt = nullptr; float* ce_tl = nullptr;
        if (ce) {
            CK(hipMalloc(&ce_part, (size_t)sh.M * nparts * sizeof(float2))); CK(hipMalloc(&ce_tgt, (size_t)sh.M * 4)); CK(hipMalloc(&ce_tl, (size_t)sh.M * 4));
            std::vector<int> t(sh.M);
            for (int i = 0; i < sh.M; ++i) t[i] = (int)((i * 2654435761u >> 8) % (unsigned)nvocab);
            CK(hipMemcpy(ce_tgt, t.data(), (size_t)sh.M * 4, hipMemcpyHostToDevice));
        }
        if (verify && !ce) {
            CK(hipMalloc(&Cref, cn * 4)); CK(hipMalloc(&csref, sh.N * 4));
            hipLaunchKernelGGL(k_ref, dim3((unsigned)((cn + 255) / 256)), dim3(256), 0, s, A, (sh.amode == OP_KC) ? sh.K : sh.M, sh.amode,
                               B, (sh.bmode == OP_KC) ? sh.K : sh.N, sh.bmode, Cref, sh.M, sh.N, sh.K, bias);
            if (sh.colsum) hipLaunchKernelGGL(k_ref_colsum, dim3((sh.N + 255) / 256), dim3(256), 0, s, B, sh.N, csref, sh.N, sh.K);
            CK(hipStreamSynchronize(s));
        }
        // ksplit 0 = sweep
        for (int S = (sh.ksplit ? sh.ksplit : 1); S <= (sh.ksplit ? sh.ksplit : (sh.K < 256 ? 3 : (sh.M < 1000 && sh.N < 1000 ? 16 : 8))); ++S) {
            GemmArgs g{};
            g.A = A; g.lda = (sh.amode == OP_KC) ? sh.K : sh.M;
            g.B = B; g.ldb = (sh.bmode == OP_KC) ? sh.K : sh.N;
            g.C = (S > 1) ? slabs : C; g.ldc = sh.N; g.M = sh.M; g.N = sh.N; g.K = sh.K;
            g.ksplit = S; g.c_slab = (long long)cn; g.bx3 = bx3;
            g.group_m = getenv("GROUP_M") ? atoi(getenv("GROUP_M")) : 0;
            g.bias = bias;
            if (ce) {
                g.nt_store = 1; g.ce_part = ce_part; g.ce_nvocab = nvocab;
                if (epi == 2) { g.ce_tgt = ce_tgt; g.ce_tgt_logit = ce_tl; } else g.ce_store = 1;
            }
            if (sh.colsum) { g.colsum = (S > 1) ? csl : cs; g.colsum_slab = sh.N; }
            float ms_k = 0, ms_t = 0;
            for (int r = -2; r < reps; ++r) {
                if (xcd_first != 0) CK(hipMemsetAsync(ctl, 0, 4 * 65536, s));
                CK(hipEventRecord(e0, s));
                if (xcd_first != 0) {
                    GemmArgs r1 = g; r1.xcd_first = xcd_first; r1.work = ctl; r1.work_limit = 1 << 30; r1.stop = ctl + 2; r1.claim = ctl + 4;
                    if (xcd_first > 0) CK(launch_gemm(s, sh.amode, sh.bmode, r1, pad));
                    r1.xcd_first = -1;
                    CK(launch_gemm(s, sh.amode, sh.bmode, r1, pad));
                } else {
                    CK(launch_gemm(s, sh.amode, sh.bmode, g, pad));
                }
                CK(hipEventRecord(e1, s));
                if (S > 1) {
                    CK(launch_reduce_slabs(s, slabs, (long long)cn, S, C, (long long)cn));
                    if (sh.colsum) CK(launch_reduce_slabs(s, csl, sh.N, S, cs, sh.N));
                }
                CK(hipEventRecord(e2, s));
                CK(hipEventSynchronize(e2));
                float a, b; CK(hipEventElapsedTime(&a, e0, e1)); CK(hipEventElapsedTime(&b, e0, e2));
                if (r >= 0) { ms_k += a; ms_t += b; }
            }
            ms_k /= reps; ms_t /= reps;
            const int tiles = bx3 == 3 ? ((sh.M + 255) / 256) * ((sh.N + 255) / 256) : ((sh.M + gemm_tile_m() - 1) / gemm_tile_m()) * ((sh.N + 127) / 128);
            if (verify && !ce) {
                CK(hipStreamSynchronize(s));
                const double e = max_rel(C, Cref, cn), ec = sh.colsum ? max_rel(cs, csref, sh.N) : 0.0;
                printf("  verify S %d: C max err / max|C| %.2e  rms err / rms %.2e  colsum err %.2e  %s\n", S, e, rms_rel(C, Cref, cn), ec, (e < 2e-5 && ec < 2e-4) ? "ok" : "MISMATCH");
                CK(hipMemset(C, 0xff, cn * 4));
            }
            if (epi) printf("EPI %d%s ", epi, (epi >= 2 && !ce) ? " (plain here)" : "");
            printf("%s  M %5d N %5d K %5d  S %d  blocks %5d (%.2f rounds of %d)  gemm %.3f ms  total %.3f ms  %.1f TF\n", sh.name, sh.M, sh.N, sh.K, S,
                   tiles * S, tiles * S / (256.0 * bpc), 256 * bpc, ms_k, ms_t, 2.0 * sh.M * sh.N * sh.K / (ms_t * 1e-3) / 1e12);
            if (getenv("PROF") && atoi(getenv("PROF")) && bx3 && xcd_first == 0) profile_launch(s, sh.amode, sh.bmode, g, pad, tiles * S, ms_k);
        }
        CK(hipFree(A)); CK(hipFree(B)); CK(hipFree(C)); CK(hipFree(cs));
        if (Cref) { CK(hipFree(Cref)); CK(hipFree(csref)); }
        if (bias) CK(hipFree(bias));
        if (ce) { CK(hipFree(ce_part)); CK(hipFree(ce_tgt)); CK(hipFree(ce_tl)); }
    }
    return 0;
}
