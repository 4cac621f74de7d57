// One translation unit per (hidden width, depth): compile with -DLNR_HT=<n_neurons/16> -DLNR_NH=<n_hidden_layers>.
// Host dispatch of mlp_backward_regs_kernel (lnr_density_regs.h) over the first layer's K blocks, the weights' home and the activation.
#include "lnr_density_regs.h"

#if !defined(LNR_HT) || !defined(LNR_NH)
#error "compile with -DLNR_HT=4|8|16 -DLNR_NH=1|2|3"
#endif
#define LNR_CAT4_(a, b, c, d) a##b##c##d
#define LNR_CAT4(a, b, c, d) LNR_CAT4_(a, b, c, d)

template <int KT1M, int WM, int ACT>
static int launch_regs(const MlpArgs& a) {
    auto kernel = mlp_backward_regs_kernel<LNR_HT, LNR_NH, KT1M, WM, ACT>;
    const size_t lds = a.route->lds;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        lnr_set_error("lnr_density_backward: hipFuncSetAttribute(%zu) failed: %s", lds, hipGetErrorString(e));
        return LNR_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kernel, dim3(a.route->grid), dim3(LNR_DENSITY_BLOCK), lds, a.st, *a.spec, a.params, a.feat, a.m_pad, a.pt->n_points, a.pt->n_rays_dev,
                       a.pt->n_rays, a.pt->n_samples, a.d_sigma, a.dfeat, a.slabs, a.want_dfeat);
    return LNR_OK;
}

template <int KT1M>
static int launch_regs_k(const MlpArgs& a) {
    const bool relu = a.spec->activation == LNR_ACT_RELU, sine = a.spec->activation == LNR_ACT_SINE;
#define LNR_REGS_GO(WM) (relu ? launch_regs<KT1M, WM, LNR_ACT_RELU>(a) : sine ? launch_regs<KT1M, WM, LNR_ACT_SINE>(a) : launch_regs<KT1M, WM, -1>(a))
    if (a.route->w_lds == 1) return LNR_REGS_GO(1);
#if LNR_NH > 1
    if (a.route->w_lds == 2) return LNR_REGS_GO(2);
#endif
    return LNR_REGS_GO(0);
#undef LNR_REGS_GO
}

int LNR_CAT4(lnr_mlp_bwd_regs_ht, LNR_HT, _nh, LNR_NH)(const MlpArgs& a) {
    const int kt1 = a.spec->in_dim / 16;
    if (kt1 <= 2) return launch_regs_k<2>(a);
    if (kt1 <= 5) return launch_regs_k<5>(a);
    return launch_regs_k<8>(a);
}
