// gram_launch.hpp — Gram matrices of the tangent sweep's vectors (gram_kernels.hpp): the workspace region of the block partials behind
// the tangent sweep's regions, and the two launches of one save point.
#pragma once

namespace {

// blocks of k_tangent_gram per trajectory: 256 amplitudes each, capped like the sweep's other reductions
unsigned gram_blocks(const Plan& pl) { return unsigned(std::min<size_t>((pl.dim + 255) / 256, 1024)); }

struct GeometryLayout {
    TangentLayout tangent;
    size_t off_partial = 0;  // [blocks][B][(1 + Dp)^2] doubles
    size_t total = 0;
};

GeometryLayout geometry_layout(const Plan& pl, const TangentLayout& t, int n_dir) {
    const int np = 1 + tangent_padded(n_dir);
    GeometryLayout g;
    g.tangent = t;
    g.off_partial = align_up(t.total);
    g.total = align_up(g.off_partial + size_t(gram_blocks(pl)) * pl.B * np * np * sizeof(double));
    return g;
}

template <int D>
void launch_tangent_gram_n(const double2* vec, size_t vstride, double* partial, uint32_t dim, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_tangent_gram<D>), grid, dim3(256), 0, stream, vec, vstride, partial, dim);
}

// G(t_k) of vec = [1 + Dp][B][dim] into gram_out[k]: [B][1 + n_dir][1 + n_dir] complex128, every entry written
int launch_gram(const Runtime& rt, char* ws, const GeometryLayout& lay, const double2* vec, int n_dir, int k, double2* gram_out,
                hipStream_t stream) {
    const Plan& pl = rt.pl;
    const int Dp = tangent_padded(n_dir), n = 1 + n_dir;
    const size_t vstride = size_t(pl.B) * pl.dim;
    double* partial = reinterpret_cast<double*>(ws + lay.off_partial);
    const unsigned nb = gram_blocks(pl);
    const dim3 grid(nb, unsigned(pl.B));
    switch (Dp) {
        case 1: launch_tangent_gram_n<1>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 2: launch_tangent_gram_n<2>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 3: launch_tangent_gram_n<3>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 4: launch_tangent_gram_n<4>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 6: launch_tangent_gram_n<6>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        case 8: launch_tangent_gram_n<8>(vec, vstride, partial, uint32_t(pl.dim), grid, stream); break;
        default: return fail(RYDIFF_EINVAL, "internal: n_dir out of range");
    }
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gram_finish, dim3(unsigned(n * n), unsigned(pl.B)), dim3(64), 0, stream, partial, int(nb), 1 + Dp, n,
                       gram_out + size_t(k) * pl.B * n * n);
    LAUNCH_CHECK();
    return RYDIFF_OK;
}

}  // namespace
