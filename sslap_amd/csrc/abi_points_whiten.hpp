// abi_points_whiten.hpp -- the launches of the whitened points calls (include/misslap.h):
//   misslap_solve_points_batch_whitened, misslap_points_batch_candidates_whitened
// The entry points share the call paths of the plain ones (points_batch_call in abi_points_batch.hpp,
// points_candidates_call in abi_points_candidates.hpp: the same argument checks, modes, workspace and uploads, plus
// points_whiten_check on w); what differs is which kernels are launched, and that is here, behind the kernels of
// kernels_points_whiten.hpp.
// (part of the single translation unit misslap.hip; included in the order given there, behind everything else)
#pragma once

namespace {
template <class T, bool Out>
struct PointsKernels<T, Out, 1> {
    static PointsWhitenCheckArgs check_args(const PointsCheckArgs &k, const WhitenView &w) { return PointsWhitenCheckArgs{k, w}; }
    static PointsWhitenArgs solve_args(const WhitenView &w) { return PointsWhitenArgs{PointsBatchArgs{}, w}; }
    static PointsBatchArgs &inner(PointsWhitenArgs &a) { return a.a; }
    static constexpr auto check = k_points_whiten_check<T, Out>;
    static constexpr auto solve = k_points_whiten_solve<T, Out>;
};

int points_whiten_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    return points_enqueue_wh<1>(st, opt, c, ws, d);
}

int points_whiten_candidates_launch(hipStream_t st, const PointsCandidatesArgs &a, const WhitenView &w, bool f32) {
    const PointsWhitenCandidatesArgs wa{a, w};
    if (f32)
        hipLaunchKernelGGL(k_points_whiten_candidates<float>, points_candidates_grid(a), dim3(kPointsCandidatesThreads), 0, st, wa);
    else
        hipLaunchKernelGGL(k_points_whiten_candidates<double>, points_candidates_grid(a), dim3(kPointsCandidatesThreads), 0, st, wa);
    HIP_TRY(hipGetLastError());
    return MISSLAP_OK;
}
}  // namespace
