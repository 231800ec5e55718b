// Which 128 x 64 sub-tile of a 256 x 256 block tile each of k_gemm_bx3h's eight waves computes, and whether that sub-tile
// holds anything of the M x N result at all.  Pure arithmetic on the tile's live extent: tests/cpp/gemm_edge_check.cpp walks
// every extent on the host.
//
// Sub-tile (wm, wn) covers rows 128 wm .. 128 wm + 127 and columns 64 wn .. 64 wn + 63 of the block tile; it is LIVE when it
// has at least one element inside the tile's live rows x live columns.  Wave w runs on SIMD w & 3, two waves per SIMD.
//   more than four live sub-tiles: the plain map (wm = w >> 2, wn = w & 3) -- a full tile gets exactly this -- and the waves of
//     dead sub-tiles are only marked;
//   at most four: the live sub-tiles go to waves 0 .. nl - 1, one per SIMD, the dead ones to the waves behind them.  With one
//     live row half the plain map already is that (sub-tile (0, wn) on wave wn); with both row halves live and at most 128
//     live columns the two row halves of a column slice would share SIMD wn, so wave w takes (w & 1, 2 (w >> 2) + ((w >> 1) & 1)).
// Either way the map is a permutation of the eight sub-tiles: every element of the tile keeps exactly one wave.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSMG_EDGE_HD __host__ __device__
#else
#define FSMG_EDGE_HD
#endif

struct GemmEdgeWave {
    int wm, wn;      // sub-tile: rows 128 wm ..., columns 64 wn ... of the block tile
    bool live;       // it holds at least one element of the result
};

// lr, lc: live rows / columns of the block tile, min(256, M - m0) and min(256, N - n0), both in [1, 256]
FSMG_EDGE_HD constexpr GemmEdgeWave gemm_edge_wave(int lr, int lc, int wave) {
    const int nlr = (lr + 127) / 128, nlc = (lc + 63) / 64;
    const bool remap = nlr == 2 && nlc <= 2;             // the one case of nl <= 4 where the plain map pairs live waves on a SIMD
    const int wm = remap ? (wave & 1) : (wave >> 2) & 1;
    const int wn = remap ? 2 * (wave >> 2) + ((wave >> 1) & 1) : wave & 3;
    return GemmEdgeWave{wm, wn, wm < nlr && wn < nlc};
}
