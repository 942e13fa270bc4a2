// The shared-phase trajectory kernel families (k_traj_tiles / split / stream / flat / quad / pipe) behind one template
// launcher per MP type.  Built once per MP type (-DMPK_MP_UNIT=0 promp, 1 dmp, 2 prodmp) so that the ~300 instantiations
// compile on several cores; without MPK_MP_UNIT (the single-unit build mpk_kernels.hip) all three are instantiated here.
#include "mpk_traj_tiles.h"
#include "mpk_traj_stream.h"
#include "mpk_traj_flat.h"
#include "mpk_traj_quad.h"
#include "mpk_traj_pipe.h"
#include "mpk_traj_route.h"

namespace mpk {

#ifndef MPK_DEVICE_ONLY
// the route's family with the call's (MP, CT) pair; the `if constexpr` guards keep the pairs a family never sees from being instantiated
template <int MP, int CT>
static int launch_traj_t(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void* stream) {
    // (full_lds: the kernels whose dynamic LDS can pass 48 KB -- k_traj_stream's bulk form only with the "lds_pad" occupancy knob)
    auto go = [&](auto kern, unsigned threads, bool full_lds = false) {
        if (full_lds && r.lds > 48 * 1024) (void)allow_full_lds(kern);
        hipLaunchKernelGGL(kern, dim3(r.blocks), dim3(threads), r.lds, (hipStream_t)stream, ta, aa);
    };
    with_km(ta.c.KP / 4, [&](auto km) {
        constexpr int KM = decltype(km)::value;
        switch (r.family) {
            case TrajFamily::Pipe:
                if constexpr (MP != MPK_MP_DMP && CT >= 3) {
                    if (r.gate) go(k_traj_pipe<MP, CT, KM, false, true>, 320);
                    else if (r.lean) go(k_traj_pipe<MP, CT, KM, true>, 320);
                    else go(k_traj_pipe<MP, CT, KM, false>, 320);
                }
                break;
            case TrajFamily::Flat:
                if constexpr (MP != MPK_MP_DMP && CT < 3) go(k_traj_flat<MP, CT, KM>, 256, true);
                break;
            case TrajFamily::Split:
                if constexpr (MP != MPK_MP_DMP && CT >= 3)
                    with_flag(r.write_through, [&](auto wt) { go(k_traj_split<MP, CT, KM, decltype(wt)::value>, 256); });
                break;
            case TrajFamily::Quarter:
                if constexpr (MP == MPK_MP_DMP || CT >= 3) {
                    if (r.nq == 1) go(k_traj_quad<MP, CT, KM, 1>, 256);
                    else if (r.nq == 2) go(k_traj_quad<MP, CT, KM, 2>, 256);
                    else go(k_traj_quad<MP, CT, KM, 4>, 256);
                }
                break;
            case TrajFamily::Stream:
                with_flag(r.bulk, [&](auto bulk) { go(k_traj_stream<MP, CT, KM, decltype(bulk)::value>, 256, decltype(bulk)::value); });
                break;
            case TrajFamily::Tiles:
                if constexpr (MP != MPK_MP_DMP && CT < 3)
                    with_flag(r.write_through, [&](auto wt) { go(k_traj_tiles<MP, CT, KM, decltype(wt)::value>, (unsigned)ta.wpb * 64u); });
                break;
            default: break;       // (the ring unit's families: mpk_traj_ring.hip)
        }
    });
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}

template <int MP>
int launch_traj_ct(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void* stream) {
    auto go = [&](auto ct) { return launch_traj_t<MP, decltype(ct)::value>(ta, aa, r, stream); };
    if constexpr (MP == MPK_MP_DMP) return go(std::integral_constant<int, -1>());
    // (the closed-loop-only families take a controller they do not know as the position controller)
    else return r.family == TrajFamily::Pipe || r.family == TrajFamily::Split ? with_closed_ct(r.ct, go) : with_ct(r.ct, go);
}

#ifdef MPK_MP_UNIT
template int launch_traj_ct<MPK_MP_UNIT>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);
#else
template int launch_traj_ct<MPK_MP_PROMP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);
template int launch_traj_ct<MPK_MP_DMP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);
template int launch_traj_ct<MPK_MP_PRODMP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);
#endif
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
