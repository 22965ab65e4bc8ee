#pragma once
// wx_lattice_fold.h -- the full-depth inverse (L = 12) of wx_lattice_dev.h with its deepest levels folded into one matrix per node.
//
// Levels 10, 11 and 12 act on nodes of 4, 2 and 1 pairs.  On a node of M pairs the one-pair advances of the odd channel wrap every M
// steps, so the NS rotations of a level go round such a node NS / M times: the lattice spends NS FMAs per sample and level on an
// operator that is periodic within the node.  In layout C these levels are lat_level<K, 0, NS, true> with K = 3, 4, 5: lane-local
// (H = 0: lat_nbr is a renaming), and the NF = 8 registers {s + 8 j} of a lane are closed under K = 3, 4, 5 (the 4 registers
// {s + 16 j} under K = 4, 5; the 2 registers {s, s + 32} under K = 5).  The composite is one NF x NF matrix, the same for every s and
// every lane: NF FMA-class instructions per sample instead of NS * log2(NF).  The host builds it by running the very recurrence on
// unit vectors (wx_lattice_fold_matrix, wx_lattice.hip), so it is in the lattice's own gain convention: lat_load_c before it and
// the levels after it are the general kernel's.
//
// Per signal and lane at NS = 8: 6144 lattice FMAs become 4608 + 512 (NF = 8), 5120 + 256 (NF = 4), 5632 + 128 (NF = 2).
#include "wx_lattice_dev.h"

#ifndef WX_LAT_FOLD
#define WX_LAT_FOLD 8     // node size NF of the fold the 4096-sample launcher uses.  Config 2 inverse leg, one MI355X: 0.977 / 0.936 / 0.910 ms for
                          // NF = 2 / 4 / 8 against 1.030 ms without the fold, none of them with scratch (profiles/fold_cfg2.md)
#endif

// row-major: new x[s + G i] = sum_j m[NF i + j] * x[s + G j], G = 64 / NF.  An argument of the folding kernels only: WxLat is passed
// by value to every lattice kernel and does not grow.
template <int NF> struct WxLatFold {
    double m[NF * NF];
};

// the matrix of levels 12 .. 13 - log2(NF) on one node (inverse: synthesis order K = 5, 4, ..; forward: analysis order), from the
// rounded shear coefficients the device uses, accumulated in long double; false = decline the fold (an entry is not finite or so
// large that the products could leave the range the lattice keeps its intermediates in)
bool wx_lattice_fold_matrix(const WxLat &cf, int NS, int NF, bool inverse, double *m);
int wx_lattice_no_fold();        // test hook (wx_debug_set_dispatch(3), wx_debug.h): the lattice kernels without the fold

namespace {

// Dense rows, RB = 4 at a time: the 4 NF coefficients of a row block are wave-uniform scalars (32 SGPR pairs for NF = 8; the whole
// 8 x 8 at once would be 128 scalar registers), the products of all but the last block wait in registers until the last block has
// read the inputs: 128 + 64 + 8 data registers at the peak for NF = 8, no temporaries beyond one node for NF <= 4.
template <int NF> __device__ __forceinline__ void lat_fold_nodes(double (&c)[64], const WxLatFold<NF> &fm)
{
    constexpr int G = 64 / NF, RB = NF < 4 ? NF : 4, NB = NF / RB;
    double t[NB > 1 ? (NB - 1) * G * RB : 1];
    lat_for<NB>([&](auto Bc) {
        constexpr int b = Bc;
        lat_for<G>([&](auto Sc) {
            constexpr int s = Sc;
            double o[RB];
            lat_for<RB>([&](auto Ic) {
                constexpr int row = RB * b + Ic;
                double acc = fm.m[NF * row] * c[s];
                lat_for<NF - 1>([&](auto Jc) {
                    constexpr int j = Jc + 1;
                    acc = fma(fm.m[NF * row + j], c[s + G * j], acc);
                });
                o[Ic] = acc;
            });
            if constexpr (b + 1 < NB) {
                lat_for<RB>([&](auto Ic) { t[(b * G + s) * RB + Ic] = o[Ic]; });
            } else {
                lat_for<NB - 1>([&](auto Pc) {
                    lat_for<RB>([&](auto Ic) { c[s + G * (RB * Pc + Ic)] = t[(Pc * G + s) * RB + Ic]; });
                });
                lat_for<RB>([&](auto Ic) { c[s + G * (RB * b + Ic)] = o[Ic]; });
            }
        });
    });
}

// lat_inv_to_l0 for L = 12.  The depth is a constant here: no switch over lat_load_c<L> and no `if (L > k)` chain.  Inside that
// control flow the merges of the 64 live registers made every form of the fold spill (33 .. 246 registers at the budget of two
// wavefronts per SIMD); in straight-line code none does.
template <int NS, int NF, typename TM, typename SINK>
__device__ __forceinline__ void lat_inv12_to_l0(const TM *__restrict__ xs, unsigned lds0, int lane, const WxLat &cf,
                                                const WxLatFold<NF> &fm, SINK &&sink)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "levels 12, 11 + 12, 10 + 11 + 12");
    double c[64];
    lat_load_c<12>(c, lds0, xs, lane, cf);
    lat_fold_nodes<NF>(c, fm);
    if constexpr (NF < 4) lat_level<4, 0, NS, true>(c, cf);
    if constexpr (NF < 8) lat_level<3, 0, NS, true>(c, cf);
    lat_level<2, 0, NS, true>(c, cf);
    lat_level<1, 0, NS, true>(c, cf);
    lat_level<0, 0, NS, true>(c, cf);
    lat_inv_c_to_l0<NS>(c, lds0, lane, cf, sink);
}

template <int NS, int WPE, int NF>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_lat_iwpt12_f64(
    const double *__restrict__ xw, double *__restrict__ y, int64_t batch, int64_t in_stride, WxLat cf, WxLatFold<NF> fm)
{
    __shared__ double lds[WX_LAT_LDS];
    const unsigned lds0 = (unsigned)(uintptr_t)(double __attribute__((address_space(3))) *)lds;
    const int lane = threadIdx.x;
    const int64_t sig = blockIdx.x;
    const unsigned yo = 64u * (lane >> 3) + 2u * (lane & 7);
    double *ys = y + sig * 4096;
    lat_inv12_to_l0<NS, NF>(xw + sig * in_stride, lds0, lane, cf, fm, [&](auto Fq, lat_d2 (&o)[8]) {
        constexpr int f = decltype(Fq)::value;
        lat_for<8>([&](auto Hq) {
            constexpr int hi3 = Hq;
            lat_st2(lat_sbase(ys + 512 * hi3 + 16 * f) + yo, o[hi3]);
        });
    });
}

}  // namespace
