// What the route choice of a shared-phase launch (plan_traj_shared / plan_episode_return, mpk_traj_launch.hip) hands to the template
// launchers of mpk_traj_family.hip, mpk_traj_ring.hip and mpk_episode.hip: the route as a value, the launchers' declarations (one
// translation unit per MP type defines them) and the helpers that turn a route's runtime facts into template arguments.
#pragma once
#include "mpk_tile.h"

namespace mpk {

// one value per kernel family a shared-phase launch can end in
enum class TrajFamily : int {
    Tiles,        // k_traj_tiles: tile-major
    Split,        // k_traj_split: tile-major with a serial role
    Stream,       // k_traj_stream: episode-major, one group per wave (bulk: chunked input staging)
    Flat,         // k_traj_flat: whole-trajectory images
    FlatD,        // k_traj_flat_d: ... with the DoF count compiled in (5 / 7 DoF, <= 8 columns; TrajArgs::burst == 2)
    Burst,        // k_traj_burst: the ring's work as short-lived workgroups (TrajArgs::burst == 1)
    Quarter,      // k_traj_quad / duo / mono: nq = 4 / 2 / 1 groups per wave, recurrences on the lane quarters
    Pipe,         // k_traj_pipe: producer / consumer workgroups
    RingOpen,     // k_traj_ring: store engine, open loop
    RingClosed,   // k_traj_ring<.., closed>: ... with consumer waves
};

struct TrajRoute {
    TrajFamily family;
    int ct;                 // fused controller: -1 none, MPK_CTRL_* open loop, 3 + MPK_CTRL_* closed loop
    bool write_through;     // Tiles / Split: the store policy is a template parameter there (episode-major kernels: TrajArgs::wt)
    bool bulk;              // Stream
    int nq;                 // Quarter: groups per wave
    bool lean, gate;        // Pipe: the register-lean instantiation / the consumer's chain with the GATE hook (which has no lean form)
    int blocks;
    size_t lds;             // dynamic LDS (Tiles / Split: the "lds_pad" occupancy padding)
    const char* name;       // what mpk_last_kernel reports: static storage
};

// k_episode_return's launch geometry
struct EpRoute {
    int ct, nq, rwd, blocks;
    size_t lds;
    const char* name;
};

#ifndef MPK_DEVICE_ONLY
// the route choice (mpk_traj_launch.hip): the request of launch_traj_shared / launch_episode_return (mpk_internal.h) and, of the launch
// site, what a rule reads -- never the stream; they fill value-initialised arguments and the route, call nothing of the HIP runtime and
// allocate nothing.  MPK_OK, or the code the launch returns without launching (a route's name is set as soon as its kernel is known,
// also where the plan then declines)
int plan_traj_shared(const DevCfg& c, const SharedTables& st, const TrajRequest& q, int num_cu, const Tuning& tune, unsigned* ticket,
                     int* fault, TrajArgs& ta, ActArgs& aa, TrajRoute& r);
int plan_episode_return(const DevCfg& c, const SharedTables& st, const TrajRequest& q, int num_cu, const Tuning& tune, TrajArgs& ta,
                        ActArgs& aa, EpArgs& ea, EpRoute& r);

template <int MP>
int launch_traj_ct(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void* stream);      // mpk_traj_family.hip
template <int MP>
int launch_traj_ring(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void* stream);    // mpk_traj_ring.hip
template <int MP>
int launch_episode_kernel(const TrajArgs& ta, const ActArgs& aa, const EpArgs& ea, const EpRoute& r, void* stream);   // mpk_episode.hip
#ifndef MPK_AMALGAMATED
#define MPK_ROUTE_LAUNCHERS(MP)                                                                                         \
    extern template int launch_traj_ct<MP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);                   \
    extern template int launch_traj_ring<MP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);                 \
    extern template int launch_episode_kernel<MP>(const TrajArgs&, const ActArgs&, const EpArgs&, const EpRoute&, void*);
MPK_ROUTE_LAUNCHERS(MPK_MP_PROMP)
MPK_ROUTE_LAUNCHERS(MPK_MP_DMP)
MPK_ROUTE_LAUNCHERS(MPK_MP_PRODMP)
#undef MPK_ROUTE_LAUNCHERS
#endif

// the launcher template of a handle's MP type: by_mp_type(mp, [&](auto mp_tag) { return launch_x<decltype(mp_tag)::value>(..); })
template <typename F>
int by_mp_type(int mp_type, F&& f) {
    switch (mp_type) {
        case MPK_MP_PRODMP: return f(std::integral_constant<int, MPK_MP_PRODMP>());
        case MPK_MP_PROMP: return f(std::integral_constant<int, MPK_MP_PROMP>());
        default: return f(std::integral_constant<int, MPK_MP_DMP>());
    }
}

// contraction columns / 4 as a compile-time constant (1 .. 4; anything else takes 4)
template <typename F>
void with_km(int km, F&& f) {
    switch (km) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        default: f(std::integral_constant<int, 4>()); break;
    }
}

// a template's bool parameter
template <typename F>
void with_flag(bool on, F&& f) {
    if (on) f(std::true_type()); else f(std::false_type());
}

// a closed-loop controller (3 + MPK_CTRL_*) as a compile-time constant; anything else takes the position controller
template <typename F>
int with_closed_ct(int ct, F&& f) {
    switch (ct) {
        case 3 + MPK_CTRL_MOTOR: return f(std::integral_constant<int, 3 + MPK_CTRL_MOTOR>());
        case 3 + MPK_CTRL_VELOCITY: return f(std::integral_constant<int, 3 + MPK_CTRL_VELOCITY>());
        default: return f(std::integral_constant<int, 3 + MPK_CTRL_POSITION>());
    }
}

// any fused controller as a compile-time constant; anything else takes -1 (none)
template <typename F>
int with_ct(int ct, F&& f) {
    switch (ct) {
        case MPK_CTRL_MOTOR: return f(std::integral_constant<int, MPK_CTRL_MOTOR>());
        case MPK_CTRL_VELOCITY: return f(std::integral_constant<int, MPK_CTRL_VELOCITY>());
        case MPK_CTRL_POSITION: return f(std::integral_constant<int, MPK_CTRL_POSITION>());
        case 3 + MPK_CTRL_MOTOR: case 3 + MPK_CTRL_VELOCITY: case 3 + MPK_CTRL_POSITION: return with_closed_ct(ct, f);
        default: return f(std::integral_constant<int, -1>());
    }
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
