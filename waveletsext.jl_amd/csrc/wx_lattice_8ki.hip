// wx_lattice_8ki.hip -- launchers of the one-pass 8192-sample kernels (wx_lattice_8k.h), inverse
#include "wx_lattice_8k.h"
#include "wx_lattice_fold.h"
bool wx_lattice_factor(const WxFilt &filt, int L, bool inverse, WxLat *out);

namespace {
// k_lat_iwpt8k_f64 with 12 levels below the first and the deepest of them folded (lat_inv12_to_l0): 8192 samples at full depth 13
template <int NS, int WPE, int NF>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_lat_iwpt8k12_f64(
    const double *__restrict__ xw, double *__restrict__ y, int64_t batch, int64_t in_stride, WxLat cf, WxFilt filt, WxLatFold<NF> fm)
{
    __shared__ double lds2[2][WX_LAT_LDS];
    __shared__ __attribute__((aligned(16))) double xch[2][2][512 + 16];   // [chunk parity][child][HB + 512 (a) | 512 + HB (d)]
    const int child = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const unsigned lds0 = (unsigned)(uintptr_t)(double __attribute__((address_space(3))) *)lds2[child];
    const int64_t sig = blockIdx.x;
    lat_d2 o[32];
    lat_inv12_to_l0<NS, NF>(xw + sig * in_stride + 4096 * child, lds0, lane, cf, fm, [&](auto Fq, lat_d2 (&oo)[8]) {
        constexpr int f = decltype(Fq)::value;
        lat_for<8>([&](auto Hq) { o[4 * Hq + f] = oo[Hq]; });
    });
    lat8k_synth<2 * NS>(o, xch, child, lane, y + sig * 8192, filt);
}
}  // namespace
// xw: leaves of signal b at xw + b in_stride (dense or the last column of packet tables), y: (8192, batch)
int wx_lattice_iwpt8k_f64(const double *xw, double *y, int L, int64_t batch, int64_t in_stride, const WxFilt &filt, hipStream_t st)
{
    if (L < 7 || L > 13 || filt.F < 2 || filt.F > 20 || batch <= 0 || batch > 0x7fffffff || xw == y) return 0;
    if ((reinterpret_cast<uintptr_t>(xw) | reinterpret_cast<uintptr_t>(y)) & 31) return 0;
    if (in_stride < 8192 || (in_stride & 3)) return 0;
    WxLat cf;
    if (!wx_lattice_factor(filt, L - 1, true, &cf)) return 0;
    // 12 levels below the first, 6 and more rotations: the deepest two folded into a 4 x 4 matrix per node (wx_lattice_fold.h; the 8 x 8 of
    // the 4096-sample kernel does not fit beside the 128 registers that hold the child's samples: 5 spilled SGPRs at 16 taps, scratch at 20)
    if (L == 13 && wx_lat_stages(filt.F) >= 6 && !wx_lattice_no_fold()) {
        WxLatFold<4> fm;
        if (wx_lattice_fold_matrix(cf, wx_lat_stages(filt.F), 4, true, fm.m)) {
            switch (wx_lat_stages(filt.F)) {
            case 6: hipLaunchKernelGGL((k_lat_iwpt8k12_f64<6, 2, 4>), dim3((unsigned)batch), dim3(128), 0, st, xw, y, batch, in_stride, cf, filt, fm); break;
            case 8: hipLaunchKernelGGL((k_lat_iwpt8k12_f64<8, 2, 4>), dim3((unsigned)batch), dim3(128), 0, st, xw, y, batch, in_stride, cf, filt, fm); break;
            default: hipLaunchKernelGGL((k_lat_iwpt8k12_f64<10, 2, 4>), dim3((unsigned)batch), dim3(128), 0, st, xw, y, batch, in_stride, cf, filt, fm); break;
            }
            const hipError_t ef = hipGetLastError();
            if (ef != hipSuccess) return wx_set_hip_error(ef, "lattice iwpt launch (8192 samples, folded)", __FILE__, __LINE__);
            return 1;
        }
    }
#define WX_GO8(NSS)                                                                                                      \
    case NSS: hipLaunchKernelGGL((k_lat_iwpt8k_f64<NSS, 2>), dim3((unsigned)batch), dim3(128), 0, st, xw, y, L - 1, batch, in_stride, cf, filt); break;
    switch (wx_lat_stages(filt.F)) {
        WX_GO8(1) WX_GO8(2) WX_GO8(4) WX_GO8(6) WX_GO8(8) WX_GO8(10)
    default: return 0;
    }
#undef WX_GO8
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return wx_set_hip_error(e, "lattice iwpt launch (8192 samples)", __FILE__, __LINE__);
    return 1;
}
