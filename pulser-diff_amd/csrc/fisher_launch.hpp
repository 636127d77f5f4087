// fisher_launch.hpp — classical Gram matrices of the tangent sweep's vectors (fisher_kernels.hpp): the workspace region of their block
// partials behind the geometry sweep's regions, and the two launches of one save point.
#pragma once

namespace {

struct FisherLayout {
    GeometryLayout geometry;
    size_t off_cpartial = 0;  // [blocks][B][(1 + Dp)(2 + Dp) / 2] doubles
    size_t total = 0;
};

// bytes of the partial region before rounding: one upper triangle per block (gram_blocks) and trajectory
size_t fisher_partial_bytes(const Plan& pl, int n_dir) {
    const int np = 1 + tangent_padded(n_dir);
    return size_t(gram_blocks(pl)) * pl.B * (np * (np + 1) / 2) * sizeof(double);
}

FisherLayout fisher_layout(const Plan& pl, const GeometryLayout& g, int n_dir) {
    FisherLayout f;
    f.geometry = g;
    f.off_cpartial = align_up(g.total);
    f.total = align_up(f.off_cpartial + fisher_partial_bytes(pl, n_dir));
    return f;
}

template <int D>
void launch_tangent_cfi_n(const double2* vec, size_t vstride, double* partial, uint32_t dim, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_tangent_cfi<D>), grid, dim3(256), 0, stream, vec, vstride, partial, dim);
}

// C(t_k) of vec = [1 + Dp][B][dim] into cgram_out[k]: [B][1 + n_dir][1 + n_dir] float64, every entry written
int launch_cfi(const Runtime& rt, char* ws, const FisherLayout& lay, const double2* vec, int n_dir, int k, double* cgram_out,
               hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int Dp = tangent_padded(n_dir), n = 1 + n_dir;
    const size_t vstride = size_t(pl.B) * pl.dim;
    double* partial = reinterpret_cast<double*>(ws + lay.off_cpartial);
    const unsigned nb = gram_blocks(pl);
    const dim3 grid(nb, unsigned(pl.B));
    switch (Dp) {
        case 1: launch_tangent_cfi_n<1>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 2: launch_tangent_cfi_n<2>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 3: launch_tangent_cfi_n<3>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 4: launch_tangent_cfi_n<4>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 6: launch_tangent_cfi_n<6>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 8: launch_tangent_cfi_n<8>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        default: return fail(RYDIFF_EINVAL, "internal: n_dir out of range");
    }
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cfi_finish, dim3(unsigned(n * n), unsigned(pl.B)), dim3(64), 0, stream, partial, int(nb), 1 + Dp, n,
                       cgram_out + size_t(k) * pl.B * n * n);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

}  // namespace
