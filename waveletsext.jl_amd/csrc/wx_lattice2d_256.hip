// the kernels of the 256 x 256 geometry (depth 5, two images per register column) of wx_lattice2d.h
#include "wx_lattice2d.h"

// One launch per pass, forward: the form a transform had until round 6, kept for the one geometry whose fused kernel spills (256 x 256
// forward with the 8 x 8 node matrices, and at 18 / 20 taps: wx_lattice2d_fused_launch declines those).  pass 1 / 2: the first / second
// pass of a transform, the intermediate image in the blocked layout of wx_lattice2d.h (the caller's scratch buffer, never seen outside
// the library).  0 = not applicable (the caller takes the strip kernels), 1 = launched, < 0 = error
int wx_lattice2d_launch_256(const float *src, float *dst, int64_t m, int L, int64_t batch, const WxFilt &filt, int pass, hipStream_t st)
{
    constexpr int HB = 1;
    WxLat2 cf;
    WxL2M mm;
    if (!l2_prepare<HB>(filt, L, false, cf, mm)) return 0;
    const int64_t per = 2, units = (batch + per - 1) / per;
    if (batch < per || units > 65535 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return 0;
    if ((batch & (per - 1)) && src == dst) return 0;          // the last workgroup re-does images: out of place only
    if (WX_L2D_W != 4 || (pass != 1 && pass != 2)) return 0;
    const int nsq = wx_lat_stages(filt.F);
    const dim3 grid((unsigned)(m / (16 * WX_L2D_W)), (unsigned)units), wg(64 * WX_L2D_W);
    const int last_img = (int)(batch - per);
#define WX_GO2(NSS)                                                                                                      \
    case NSS:                                                                                                            \
        if (pass == 2) hipLaunchKernelGGL((k_lat2d_colT_f32<NSS, true, false, HB>), grid, wg, 0, st, src, dst, last_img, cf, mm);   \
        else hipLaunchKernelGGL((k_lat2d_colT_f32<NSS, false, true, HB>), grid, wg, 0, st, src, dst, last_img, cf, mm);  \
        break;
    switch (nsq) {
        WX_GO2(1) WX_GO2(2) WX_GO2(4) WX_GO2(6) WX_GO2(8) WX_GO2(10)
    default: return 0;
    }
#undef WX_GO2
    WX_DWT2D_TRACE(WX_R2_L2DC, 0, 0, L, sizeof(float), grid, wg, 0, nsq, HB, pass);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return wx_set_hip_error(e, "lattice2d launch", __FILE__, __LINE__);
    return 1;
}
int wx_lattice2d_fused_256(const float *src, float *dst, float *ring, unsigned *ctl, int64_t m, int L, int64_t batch, const WxFilt &filt, bool inverse,
                          hipStream_t st)
{
    return wx_lattice2d_fused_launch<1>(src, dst, ring, ctl, m, L, batch, filt, inverse, st);
}
int64_t wx_lattice2d_ring_elems_256(int64_t batch) { return wx_lattice2d_ring_elems_t<1>(batch); }
