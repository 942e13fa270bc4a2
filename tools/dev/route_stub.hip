// Differential check of the shared-phase route choice, without a GPU: this unit is linked with ONE mpk_traj_launch.hip (the working
// tree's, or an older commit's exported with git) in place of mpk_traj_family.hip / mpk_traj_ring.hip / mpk_episode.hip and
// mpk_host.cpp.  Its launch_traj_ct / launch_traj_ring / launch_episode_kernel record their arguments instead of launching, and
// main() sweeps launch_traj_shared / launch_episode_return over shapes, call kinds, pointer alignments and options.  No kernel is
// launched and no device is opened.  tools/dev/route_diff.py builds it twice and compares the two record streams.
//
//   -DROUTE_OLD_ABI            the launchers of the commits before TrajRoute (positional flags); normalised to the same record
//   -DROUTE_POSITIONAL_CALLS   the commits before TrajRequest / LaunchSite: launch_traj_shared / launch_episode_return take argument lists
//   route_stub <shard 0..3 | all>                one line per block (MP, D, T, KP, option): case count + hash of its records
//   route_stub <shard> --dump '<block key>'      every record of that block, one per line
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mpk_tile.h"
#ifndef ROUTE_OLD_ABI
#include "mpk_traj_route.h"
#elif !defined(ROUTE_POSITIONAL_CALLS)
#define ROUTE_POSITIONAL_CALLS
#endif

namespace mpk {

static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

struct Rec {
    int n = 0;
    const char* k[192];
    long long v[192];
    void add(const char* key, long long val) { k[n] = key; v[n] = val; ++n; }
    void addd(const char* key, double d) { long long b; std::memcpy(&b, &d, 8); add(key, b); }
    void addp(const char* key, const void* p) { add(key, (long long)reinterpret_cast<uintptr_t>(p)); }
};
static Rec g_call;          // what the last stub call received; n == 0: nothing was launched

static unsigned long long fnv(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

// the ten kernel families, in the order of TrajFamily
enum { F_TILES, F_SPLIT, F_STREAM, F_FLAT, F_FLAT_D, F_BURST, F_QUARTER, F_PIPE, F_RING_OPEN, F_RING_CLOSED, F_EPISODE };

static void rec_route(const char* launcher, int mp, int family, int ct, int wt, int bulk, int nq, int lean, int gate, long long blocks,
                      size_t lds) {
    Rec& r = g_call;
    r.n = 0;
    r.add(launcher, mp);
    r.add("family", family); r.add("ct", ct); r.add("write_through", wt); r.add("bulk", bulk); r.add("nq", nq);
    r.add("lean", lean); r.add("gate", gate); r.add("blocks", blocks); r.add("lds", (long long)lds);
}

static void rec_args(const TrajArgs& ta, const ActArgs& aa) {
    Rec& r = g_call;
#define I(f) r.add(#f, (long long)ta.f)
#define P(f) r.addp(#f, ta.f)
#define D(f) r.addd(#f, ta.f)
    I(c.mp_type); I(c.phase_type); I(c.basis_type); I(c.D); I(c.nb); I(c.n_total); I(c.zs); I(c.KT); I(c.KP); I(c.P); I(c.Kloc); I(c.off);
    I(c.T); I(c.dmp_resp);
    P(A); P(aux); I(TS); P(params); P(init_pos); P(init_vel); P(pos); P(vel); P(actions); P(c_pos); P(c_vel);
    I(B); I(sh); I(G); I(vec_ok); I(pitch); I(cps); I(shifted); I(td3); I(inv_cps); I(nrt_magic); I(gstride); I(wt); I(flat_img);
    I(ring_np); I(ring_ns); I(ring_m); I(ring_nbuf); I(ring_nc); I(ring_aw); P(ring_ctr); I(ring_tb); I(ring_parts); I(burst); I(lean);
    I(inorder); I(wpb); I(ring_dbg); P(fault); I(ser_blocks); P(q_state); P(qd_state); P(n_steps); D(plant_dt);
    P(rp.traj_steps); P(rp.plan_steps); P(rp.done); P(rp.seg_len); P(rp.done_out); P(rp.cond_pos); P(rp.cond_vel);
    I(rp.every); I(rp.max_planning_times); I(rp.horizon);
    P(gate_valid); P(gate_penalty); P(gate_raw); I(gate_check_td); D(gate_tb[0]); D(gate_tb[1]); D(gate_db[0]); D(gate_db[1]);
#undef I
#undef P
#undef D
    static_assert(sizeof(ActArgs) == 6 * kMaxD * sizeof(double) + 2 * kMaxD * sizeof(float), "ActArgs has padding: hash its fields");
    r.add("act_args", (long long)fnv(&aa, sizeof(aa)));
    r.addd("pg0", aa.pg[0]); r.addd("hi0", aa.hi[0]); r.addd("glo0", aa.glo[0]); r.add("ghi32_0", (long long)(aa.ghi32[0] * 1024.0f));
}

static void rec_ep(const EpArgs& ea) {
    Rec& r = g_call;
    r.addp("ep.ret", ea.ret); r.addp("ep.goal", ea.goal); r.addp("ep.step0", ea.step0); r.addp("ep.seg_out", ea.seg_out);
    r.add("ep.steps_before_reward", ea.steps_before_reward); r.add("ep.agg", ea.agg); r.add("ep.km", ea.km); r.add("ep.wpb", ea.wpb);
}

#ifdef ROUTE_OLD_ABI
// the family the old launcher derived from its positional flags (launch_traj_ct / launch_traj_t of those commits, same precedence)
template <int MP>
int launch_traj_ct(const TrajArgs& ta, const ActArgs& aa, int ct, bool stream_mode, bool write_through, bool bulk, int quad, int blocks,
                   size_t lds, void*, bool split, bool pipe) {
    if (MP != MPK_MP_DMP && !pipe && !split && ct >= 3) { stream_mode = true; write_through = false; }   // (closed loop: episode-major)
    const int fam = pipe ? F_PIPE : ta.flat_img > 0 ? F_FLAT : split ? F_SPLIT : stream_mode && quad ? F_QUARTER : stream_mode ? F_STREAM : F_TILES;
    const bool tile_major = fam == F_TILES || fam == F_SPLIT;
    rec_route("launch_traj_ct", MP, fam, ct, tile_major && write_through, fam == F_STREAM && bulk, fam == F_QUARTER ? quad : 0,
              fam == F_PIPE && !ta.gate_valid && ta.lean, (fam == F_PIPE || fam == F_QUARTER) && ta.gate_valid, blocks, lds);
    rec_args(ta, aa);
    return MPK_OK;
}
template <int MP>
int launch_traj_ring(const TrajArgs& ta, const ActArgs& aa, int ct, int blocks, size_t lds, void*) {
    const int fam = ta.burst == 1 ? F_BURST : ta.burst == 2 ? F_FLAT_D : ct >= 3 ? F_RING_CLOSED : F_RING_OPEN;
    rec_route("launch_traj_ring", MP, fam, ct, 0, 0, 0, 0, 0, blocks, lds);
    rec_args(ta, aa);
    return MPK_OK;
}
template <int MP>
int launch_episode_kernel(const TrajArgs& ta, const ActArgs& aa, const EpArgs& ea, int ct, int nq, int rwd, int blocks, size_t lds, void*) {
    rec_route("launch_episode_kernel", MP, F_EPISODE, ct, 0, 0, nq, 0, 0, blocks, lds);
    g_call.add("rwd", rwd);
    rec_args(ta, aa);
    rec_ep(ea);
    return MPK_OK;
}
#define ROUTE_INST(MP)                                                                                                              \
    template int launch_traj_ct<MP>(const TrajArgs&, const ActArgs&, int, bool, bool, bool, int, int, size_t, void*, bool, bool);   \
    template int launch_traj_ring<MP>(const TrajArgs&, const ActArgs&, int, int, size_t, void*);                                    \
    template int launch_episode_kernel<MP>(const TrajArgs&, const ActArgs&, const EpArgs&, int, int, int, int, size_t, void*);
#else
static void rec_traj_route(const char* launcher, int mp, const TrajRoute& r) {
    static_assert((int)TrajFamily::Tiles == F_TILES && (int)TrajFamily::Split == F_SPLIT && (int)TrajFamily::Stream == F_STREAM &&
                  (int)TrajFamily::Flat == F_FLAT && (int)TrajFamily::FlatD == F_FLAT_D && (int)TrajFamily::Burst == F_BURST &&
                  (int)TrajFamily::Quarter == F_QUARTER && (int)TrajFamily::Pipe == F_PIPE && (int)TrajFamily::RingOpen == F_RING_OPEN &&
                  (int)TrajFamily::RingClosed == F_RING_CLOSED, "the record's family numbers");
    rec_route(launcher, mp, (int)r.family, r.ct, r.write_through, r.bulk, r.nq, r.lean, r.gate, r.blocks, r.lds);
}
template <int MP>
int launch_traj_ct(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void*) {
    rec_traj_route("launch_traj_ct", MP, r);
    rec_args(ta, aa);
    return MPK_OK;
}
template <int MP>
int launch_traj_ring(const TrajArgs& ta, const ActArgs& aa, const TrajRoute& r, void*) {
    rec_traj_route("launch_traj_ring", MP, r);
    rec_args(ta, aa);
    return MPK_OK;
}
template <int MP>
int launch_episode_kernel(const TrajArgs& ta, const ActArgs& aa, const EpArgs& ea, const EpRoute& r, void*) {
    rec_route("launch_episode_kernel", MP, F_EPISODE, r.ct, 0, 0, r.nq, 0, 0, r.blocks, r.lds);
    g_call.add("rwd", r.rwd);
    rec_args(ta, aa);
    rec_ep(ea);
    return MPK_OK;
}
#define ROUTE_INST(MP)                                                                                  \
    template int launch_traj_ct<MP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);          \
    template int launch_traj_ring<MP>(const TrajArgs&, const ActArgs&, const TrajRoute&, void*);        \
    template int launch_episode_kernel<MP>(const TrajArgs&, const ActArgs&, const EpArgs&, const EpRoute&, void*);
#endif
ROUTE_INST(MPK_MP_PROMP)
ROUTE_INST(MPK_MP_DMP)
ROUTE_INST(MPK_MP_PRODMP)

}  // namespace mpk

using namespace mpk;

namespace {

// made-up device addresses (never dereferenced): 16-byte aligned, `off` bytes past that on request
template <typename T>
T* fake(int slot, int off = 0) { return reinterpret_cast<T*>((uintptr_t)0x10000000u * (unsigned)(slot + 1) + (unsigned)off); }

struct Opt { std::string name; Tuning t; };

std::vector<Opt> option_sweep() {
    std::vector<Opt> v;
    v.push_back({"default", Tuning()});
    auto alone = [&](const char* key, int Tuning::*f, std::vector<int> vals) {
        for (int x : vals) { Opt o{std::string(key) + "=" + std::to_string(x), Tuning()}; o.t.*f = x; v.push_back(o); }
    };
    auto range = [](int lo, int hi) { std::vector<int> r; for (int i = lo; i <= hi; ++i) r.push_back(i); return r; };
    // every selection option of mpk_host.cpp's OptKey table that launch_traj_shared / launch_episode_return read, alone, at each
    // legal value ("ipw" 0 .. 2^20 and "ring_dbg" 0 .. 255: the boundaries, every bit the rule tests, and a few values between)
    alone("mapping", &Tuning::mapping, range(0, 2));
    alone("bulk", &Tuning::bulk, range(0, 2));
    alone("quad", &Tuning::quad, range(0, 4));
    alone("write_through", &Tuning::write_through, range(0, 1));
    alone("ipw", &Tuning::ipw, {0, 1, 2, 3, 7, 64, 4096, 1 << 20});
    alone("split", &Tuning::split, range(0, 1));
    alone("lds_pad", &Tuning::lds_pad, range(0, 48));
    alone("pipe", &Tuning::pipe, range(0, 1));
    alone("flat", &Tuning::flat, range(0, 1));
    alone("ring", &Tuning::ring, range(0, 2));
    alone("ring_np", &Tuning::ring_np, range(1, 14));
    alone("ring_ns", &Tuning::ring_ns, range(1, 8));
    alone("ring_m", &Tuning::ring_m, range(1, 8));
    alone("ring_dbg", &Tuning::ring_dbg, {0, 1, 2, 4, 8, 16, 32, 64, 128, 72, 139, 255});
    alone("ring_parts", &Tuning::ring_parts, range(1, 8));
    alone("tiles_wpb", &Tuning::tiles_wpb, range(1, 8));
    alone("serial_order", &Tuning::serial_order, range(0, 2));
    alone("ring_nc", &Tuning::ring_nc, range(1, 6));
    alone("ablations", &Tuning::ablations, range(0, 1));
    alone("ring_tb", &Tuning::ring_tb, range(1, 64));
    alone("phase_waves", &Tuning::phase_waves, range(1, 32));
    // the store-engine geometry together: forced ring (1) / burst (2) with groups per batch, producer / engine / consumer waves,
    // batches per ticket and waves per group
    for (int ring = 1; ring <= 2; ++ring)
        for (int m : {1, 2, 3, 4, 8})
            for (int np : {1, 2, 8, 14}) {
                Opt o{"", Tuning()};
                o.t.ring = ring; o.t.ring_m = m; o.t.ring_np = np; o.t.ring_ns = (m + np) % 8 + 1; o.t.ring_nc = np % 6 + 1;
                o.t.ring_tb = (m * np) % 5 == 0 ? -1 : (m * np) % 5; o.t.ring_parts = np % 4 == 0 ? -1 : np % 4;
                o.name = "ring=" + std::to_string(ring) + ",m=" + std::to_string(m) + ",np=" + std::to_string(np);
                v.push_back(o);
            }
    for (int dbg : {8, 64, 139}) {
        Opt o{"ring=1,ablations=1,ring_dbg=" + std::to_string(dbg), Tuning()};
        o.t.ring = 1; o.t.ablations = 1; o.t.ring_dbg = dbg;
        v.push_back(o);
        o.name = "flat=1,ring_dbg=" + std::to_string(dbg); o.t = Tuning(); o.t.flat = 1; o.t.ring_dbg = dbg;
        v.push_back(o);
    }
    return v;
}

const int kD[] = {1, 2, 5, 7, 8, 16}, kT[] = {2, 25, 100, 200, 1000}, kKP[] = {4, 8, 12, 16};
const int kB[] = {1, 2, 3, 15, 16, 17, 64, 255, 256, 1024, 2048, 4096, 6144, 8192, 8193, 8704, 12288, 12289, 14336, 16383, 16384,
                  18432, 32768, 49152, 65536, 131072, 262144, 524288, 1048576};
const int kCU[] = {256, 8};
const char* const kMpName[] = {"promp", "dmp", "prodmp", "dmp_resp"};

DevCfg make_cfg(int mpv, int D, int T, int KP) {
    DevCfg c;
    std::memset(&c, 0, sizeof(c));
    c.mp_type = mpv == 0 ? MPK_MP_PROMP : mpv == 1 ? MPK_MP_DMP : MPK_MP_PRODMP;
    c.dmp_resp = mpv == 3;
    c.D = D; c.T = T; c.KP = c.KT = KP;
    c.nb = c.mp_type == MPK_MP_PRODMP ? (KP > 3 ? KP - 3 : 1) : KP;
    c.n_total = c.nb;
    c.Kloc = c.nb + (c.mp_type == MPK_MP_PROMP ? 0 : 1);
    c.P = D * c.Kloc;
    c.tau = 1.5f;
    c.tab = fake<double>(20); c.rows32 = fake<float>(21); c.base_times = fake<float>(22);
    return c;
}

struct Sums {
    std::map<std::string, long> names, exits;
    long cases = 0;
};

// one case's record: return code, error text, kernel name, then what the launcher received
unsigned long long finish(int rc, const char* name, Sums& s, std::string* text) {
    unsigned long long h = fnv(&rc, sizeof(rc));
    h = fnv(g_err.data(), g_err.size(), h);
    h = fnv(name, std::strlen(name), h);
    h = fnv(&g_call.n, sizeof(int), h);
    for (int i = 0; i < g_call.n; ++i) { h ^= (unsigned long long)g_call.v[i]; h *= 1099511628211ull; h ^= h >> 29; }
    ++s.cases;
    if (rc == MPK_OK) ++s.names[name];
    else ++s.exits["rc=" + std::to_string(rc) + " err='" + g_err + "' name=" + (name[0] ? "set" : "unset")];
    if (text) {
        *text = "rc=" + std::to_string(rc) + " err='" + g_err + "' name='" + name + "'";
        for (int i = 0; i < g_call.n; ++i) *text += std::string(" ") + g_call.k[i] + "=" + std::to_string(g_call.v[i]);
    }
    return h;
}

// call kinds: 0 trajectory only, 1 open-loop actions, 2 closed loop, 3 closed loop + replanning state, 4 closed loop + gate,
// 5 closed loop + replanning state + gate (tau / delay checked, raw action given), 6 a gate without the closed loop (MPK_EINVAL),
// 7 plant state without actions
const int kKinds = 8;
// pointer alignment: 0 all 16-byte aligned, 1 outputs 4 bytes off, 2 inputs 4 bytes off
const int kAligns = 3;

unsigned long long traj_case(const DevCfg& c, const SharedTables& st, const Tuning& tune, int B, int kind, int al, int cu, Sums& s,
                             std::string* text) {
    const int oo = al == 1 ? 4 : 0, io = al == 2 ? 4 : 0;
    const bool act = kind != 0 && kind != 7, closed = kind >= 2 && kind != 6, rpl = kind == 3 || kind == 5, gated = kind >= 4 && kind <= 6;
    RolloutDev rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.controller_type = (kind + c.D) % 3; rc.plant_type = closed ? 1 : 0; rc.dt = 0.02;
    for (int d = 0; d < c.D; ++d) { rc.pg[d] = 1.0 + d; rc.dg[d] = 0.1 * (d + 1); rc.lo[d] = -1.0 - d; rc.hi[d] = 1.0 + 0.5 * d; }
    ReplanDev rp;
    rp.traj_steps = fake<int32_t>(30); rp.plan_steps = fake<int32_t>(31); rp.done = fake<uint8_t>(32); rp.seg_len = fake<int32_t>(33);
    rp.cond_pos = fake<float>(34); rp.cond_vel = fake<float>(35); rp.every = 25; rp.max_planning_times = 4; rp.horizon = c.T;
    GateDev gd;
    for (int d = 0; d < kMaxD; ++d) { gd.lo[d] = -2.0 - 0.1 * d; gd.hi[d] = 2.0 + 0.3 * d; }
    gd.valid = fake<uint8_t>(40); gd.penalty = fake<double>(41);
    if (kind == 5) { gd.check_td = 1; gd.tau_b[0] = 0.5; gd.tau_b[1] = 3.0; gd.delay_b[0] = 0.0; gd.delay_b[1] = 0.25; gd.raw_params = fake<float>(42); }
    const char* name = "";
    g_err.clear();
    g_call.n = 0;
    float* const actions = act ? fake<float>(6, oo) : nullptr;
    const double* const c_pos = act && !closed ? fake<double>(7, 2 * io) : nullptr;
    const double* const c_vel = act && !closed ? fake<double>(8, 2 * io) : nullptr;
    double* const q = closed ? fake<double>(9) : nullptr;
    double* const qd = closed ? fake<double>(10) : nullptr;
    const int32_t* const n_steps = closed && !rpl ? fake<int32_t>(11) : nullptr;
#ifdef ROUTE_POSITIONAL_CALLS
    const int r = launch_traj_shared(c, st, fake<float>(1, io), fake<float>(2, io), fake<float>(3, io), fake<float>(4, oo), fake<float>(5, oo),
                                     actions, act ? &rc : nullptr, c_pos, c_vel, q, qd, n_steps, B, cu, nullptr, &name, tune,
                                     rpl ? &rp : nullptr, fake<unsigned>(12), fake<int>(13), gated ? &gd : nullptr);
#else
    TrajRequest req;
    req.params = fake<float>(1, io); req.init_pos = fake<float>(2, io); req.init_vel = fake<float>(3, io);
    req.pos = fake<float>(4, oo); req.vel = fake<float>(5, oo); req.actions = actions; req.rc = act ? &rc : nullptr;
    req.c_pos = c_pos; req.c_vel = c_vel; req.q_state = q; req.qd_state = qd; req.n_steps = n_steps;
    req.rp = rpl ? &rp : nullptr; req.gate = gated ? &gd : nullptr; req.B = B;
    LaunchSite at;
    at.num_cu = cu; at.tune = tune; at.kernel_name = &name; at.ticket = fake<unsigned>(12); at.fault = fake<int>(13);
    const int r = launch_traj_shared(c, st, req, at);
#endif
    return finish(r, name, s, text);
}

// launch_episode_return: variant bit 0 reward, bit 1 replanning state, bit 2 gate
unsigned long long ep_case(const DevCfg& c, const SharedTables& st, const Tuning& tune, int B, int variant, int cu, Sums& s, std::string* text) {
    RolloutDev rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.controller_type = (variant + c.D) % 3; rc.plant_type = 1; rc.dt = 0.01;
    for (int d = 0; d < c.D; ++d) { rc.pg[d] = 2.0 + d; rc.dg[d] = 0.2 * (d + 1); rc.lo[d] = -1.5 - d; rc.hi[d] = 1.5 + 0.5 * d; }
    ReplanDev rp;
    rp.traj_steps = fake<int32_t>(30); rp.plan_steps = fake<int32_t>(31); rp.done = fake<uint8_t>(32); rp.seg_len = fake<int32_t>(33);
    rp.every = 10; rp.max_planning_times = 0; rp.horizon = c.T;
    GateDev gd;
    for (int d = 0; d < kMaxD; ++d) { gd.lo[d] = -3.0 - 0.1 * d; gd.hi[d] = 3.0 + 0.3 * d; }
    gd.valid = fake<uint8_t>(40);
    const bool rwd = variant & 1, rpl = variant & 2, gated = variant & 4;
    const char* name = "";
    g_err.clear();
    g_call.n = 0;
    const double* const goal = rwd ? fake<double>(14) : nullptr;
    const int32_t* const n_steps = rpl ? nullptr : fake<int32_t>(11);
    const int32_t* const step0 = rpl ? nullptr : fake<int32_t>(15);
    int32_t* const seg_out = gated ? nullptr : fake<int32_t>(17);
#ifdef ROUTE_POSITIONAL_CALLS
    const int r = launch_episode_return(c, st, fake<float>(1), fake<float>(2), fake<float>(3), rc, fake<double>(9), fake<double>(10), n_steps,
                                        rpl ? &rp : nullptr, rwd ? 1 : 0, goal, step0, 190, variant % 3, fake<double>(16), seg_out, B, cu,
                                        nullptr, &name, tune, gated ? &gd : nullptr);
#else
    TrajRequest req;
    req.params = fake<float>(1); req.init_pos = fake<float>(2); req.init_vel = fake<float>(3); req.rc = &rc;
    req.q_state = fake<double>(9); req.qd_state = fake<double>(10); req.n_steps = n_steps;
    req.rp = rpl ? &rp : nullptr; req.gate = gated ? &gd : nullptr; req.B = B;
    req.ep.reward = rwd ? 1 : 0; req.ep.goal = goal; req.ep.step0 = step0; req.ep.steps_before_reward = 190; req.ep.agg = variant % 3;
    req.ep.ret = fake<double>(16); req.ep.seg_out = seg_out;
    LaunchSite at;
    at.num_cu = cu; at.tune = tune; at.kernel_name = &name;
    const int r = launch_episode_return(c, st, req, at);
#endif
    return finish(r, name, s, text);
}

}  // namespace

int main(int argc, char** argv) {
    const int shard = argc > 1 && std::strcmp(argv[1], "all") != 0 ? std::atoi(argv[1]) : -1;
    const char* dump = argc > 3 && std::strcmp(argv[2], "--dump") == 0 ? argv[3] : nullptr;
    const std::vector<Opt> opts = option_sweep();
    std::vector<Opt> ep_opts;
    ep_opts.push_back({"default", Tuning()});
    for (int q = 2; q <= 4; ++q) { Opt o{"quad=" + std::to_string(q), Tuning()}; o.t.quad = q; ep_opts.push_back(o); }
    for (int w : {1, 4, 8}) { Opt o{"tiles_wpb=" + std::to_string(w), Tuning()}; o.t.tiles_wpb = w; ep_opts.push_back(o); }
    { Opt o{"quad=2,tiles_wpb=8", Tuning()}; o.t.quad = 2; o.t.tiles_wpb = 8; ep_opts.push_back(o); }
    Sums s;
    for (int mpv = 0; mpv < 4; ++mpv) {
        if (shard >= 0 && mpv != shard) continue;
        for (int D : kD) for (int T : kT) for (int KP : kKP) {
            const DevCfg c = make_cfg(mpv, D, T, KP);
            SharedTables st;
            (void)shared_tables_floats(c, &st.TS, &st.n_out);
            st.A = fake<float>(18); st.aux = fake<float>(19);
            const std::string shape = std::string(kMpName[mpv]) + " D=" + std::to_string(D) + " T=" + std::to_string(T) + " KP=" + std::to_string(KP) + " ";
            for (int ep = 0; ep < 2; ++ep)
                for (const Opt& o : ep ? ep_opts : opts) {
                    const std::string key = (ep ? "episode " : "traj ") + shape + o.name;
                    if (dump && key != dump) continue;
                    unsigned long long h = 1469598103934665603ull;
                    long n = 0;
                    std::string text;
                    for (int B : kB) for (int cu : kCU) for (int k = 0; k < (ep ? 8 : kKinds * kAligns); ++k) {
                        const unsigned long long hc = ep ? ep_case(c, st, o.t, B, k, cu, s, dump ? &text : nullptr)
                                                         : traj_case(c, st, o.t, B, k / kAligns, k % kAligns, cu, s, dump ? &text : nullptr);
                        h = fnv(&hc, sizeof(hc), h);
                        ++n;
                        if (dump) std::printf("B=%d cu=%d %s=%d | %s\n", B, cu, ep ? "variant" : "kind*3+align", k, text.c_str());
                    }
                    if (!dump) std::printf("BLOCK\t%s\t%ld\t%016llx\n", key.c_str(), n, h);
                }
        }
    }
    if (!dump) {
        for (const auto& kv : s.names) std::printf("NAME\t%s\t%ld\n", kv.first.c_str(), kv.second);
        for (const auto& kv : s.exits) std::printf("EXIT\t%s\t%ld\n", kv.first.c_str(), kv.second);
        std::printf("CASES\t%ld\n", s.cases);
    }
    return 0;
}
