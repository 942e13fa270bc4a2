// the launch plumbing the probabilistic units share (mpk_traj_condition.hip, mpk_traj_log_prob.hip, mpk_demo_log_prob.hip,
// mpk_demo_condition.hip, mpk_traj_phase_std.hip; mpk_traj_std.hip takes the two refusals only): host code, no kernel
#pragma once

#include "mpk_dev.h"

#ifndef MPK_DEVICE_ONLY
namespace mpk {

// what every kernel of the probabilistic interface refuses first, under the entry's name fn: a DMP, the k_traj_wide shapes
inline int gauss_common_limits(const DevCfg& c, const char* fn) {
    const std::string name(fn);
    if (c.mp_type == MPK_MP_DMP || c.dmp_resp) {
        set_error(name + ": a DMP has no probabilistic interface (promp / prodmp only)");
        return MPK_ENOTIMPL;
    }
    if (c.D > kMaxD || c.KP > kMaxKP) {
        set_error(name + ": at most " + std::to_string(kMaxD) + " DoF and " + std::to_string(kMaxKP) +
                  " table columns (this handle: " + std::to_string(c.D) + " DoF, " + std::to_string(c.KT) +
                  " columns); the k_traj_wide shapes have no kernel here");
        return MPK_ENOTIMPL;
    }
    return MPK_OK;
}

// ... and what a per-episode row source (mpk_phase_rows.h, `slots` row slots) refuses on top, in demo_phase_limits' words
inline int gauss_phase_row_limits(const DevCfg& c, int slots, const char* fn) {
    const int need = c.mp_type == MPK_MP_PRODMP ? c.nb + 3 : c.KT;
    if (need > slots || c.Kloc > slots || c.D < 1 || !c.tab) {
        set_error(std::string(fn) + ": at most " + std::to_string(kMaxD) + " DoF and " + std::to_string(kMaxKP) +
                  " table columns (this handle: " + std::to_string(c.D) + " DoF, " + std::to_string(need) +
                  " columns); the per-episode rows are those of the wave kernel k_traj_phase");
        return MPK_ENOTIMPL;
    }
    return MPK_OK;
}

// one wave per episode, wave_doubles float64 words of LDS per wave and `shared` bytes per workgroup: the waves per workgroup (<= 4) that
// put the most waves on a CU, the larger workgroup on a tie (the tables are staged once each), and the workgroup's LDS bytes.  The
// caller has refused a shape whose single wave does not fit.
struct WavePlan {
    int waves = 1;
    size_t lds = 0;
};
inline WavePlan gauss_wave_plan(size_t wave_doubles, size_t shared) {
    WavePlan p;
    size_t best_on_cu = 0;
    for (int w = 1; w <= 4; ++w) {
        const size_t bytes = w * wave_doubles * sizeof(double) + shared;
        if (bytes > kLdsPerCu) break;
        const size_t on_cu = w * (kLdsPerCu / bytes);
        if (on_cu >= best_on_cu) { p.waves = w; best_on_cu = on_cu; }
    }
    p.lds = p.waves * wave_doubles * sizeof(double) + shared;
    return p;
}

// the workgroups of B episodes: what the LDS lets a CU hold (1..8) on every CU, or one per `waves` episodes where that is fewer
inline int gauss_blocks(int B, int waves, size_t lds, int num_cu) {
    const int fit = (int)(kLdsPerCu / lds);
    const int per_cu = fit < 1 ? 1 : (fit > 8 ? 8 : fit);
    const long units = ((long)B + waves - 1) / waves;
    return (int)(units < (long)num_cu * per_cu ? units : (long)num_cu * per_cu);
}

// run-time values as template arguments: f is a generic lambda that reads its argument's ::value.  ns: rows per lane, 1..4 (a larger
// Pl has been refused); the movement primitive; a boolean template flag
template <class F>
int dispatch_ns(int ns, F&& f) {
    switch (ns) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
template <class F>
int dispatch_mp(bool promp, F&& f) {
    return promp ? f(std::integral_constant<int, MPK_MP_PROMP>{}) : f(std::integral_constant<int, MPK_MP_PRODMP>{});
}
template <class F>
int dispatch_flag(bool on, F&& f) {
    return on ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace mpk
#endif  // MPK_DEVICE_ONLY
