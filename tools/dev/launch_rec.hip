// Differential check of the rollout and learned-phase launchers (mpk_rollout.hip, mpk_phase_fused.hip, mpk_traj_phase.hip) at the
// launch boundary, without a GPU: this program includes the three units of ONE tree (the working tree's, or another commit's exported
// with git) with hipLaunchKernelGGL, hipFuncSetAttribute, hipGetDevice and hipGetLastError replaced by recorders, and sweeps
// launch_pd_rollout / launch_reacher_rollout / launch_phase_fused / launch_traj_rows over shapes, call kinds, pointer alignments and
// options.  A record holds what a launch is: the kernel's symbol, grid, block, dynamic LDS, the bytes of every by-value argument, the
// kernels whose LDS attribute was raised, the return code, the error text and *kernel_name.  No kernel runs and no device is opened
// (compile with --offload-host-only).  tools/dev/launch_diff.py builds it twice and compares the two record streams.
//
//   -DLAUNCH_POSITIONAL_CALLS   the commits before TrajRequest / LaunchSite: launch_phase_fused / launch_traj_rows take argument lists
//   launch_rec <rollout | fused | rows> <shard 0..7 | all> [--quick]     one line per block (shape, option): case count + hash of its records
//   launch_rec <unit> <shard> --dump '<block key>'                       every record of that block, one per line
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace rec {

static unsigned long long fnv(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

static std::string g_text;          // what the launcher did since the case began: "attr=<symbol>" and "launch=<symbol> ..." items
static std::map<std::string, long> g_syms;

static const std::string& symbol(const void* fn) {
    static std::unordered_map<const void*, std::string> cache;
    auto it = cache.find(fn);
    if (it != cache.end()) return it->second;
    Dl_info info;
    std::string s = dladdr(fn, &info) && info.dli_sname && info.dli_saddr == fn ? info.dli_sname : "?";
    return cache.emplace(fn, s).first->second;
}

template <class A>
static void arg_bytes(const A& a) {
    char buf[40];
    std::snprintf(buf, sizeof buf, " %zu:%016llx", sizeof(A), fnv(&a, sizeof(A)));
    g_text += buf;
}

template <class K, class... Args>
static void launch(K kern, dim3 g, dim3 b, size_t lds, hipStream_t, const Args&... args) {
    const std::string& s = symbol(reinterpret_cast<const void*>(kern));
    ++g_syms[s];
    char buf[96];
    std::snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u,%u,%u lds=%zu args", g.x, g.y, g.z, b.x, b.y, b.z, lds);
    g_text += " launch=" + s + buf;
    (arg_bytes(args), ...);
}

static hipError_t set_attr(const void* fn) { g_text += " attr=" + symbol(fn); return hipSuccess; }
static hipError_t get_device(int* dev) { *dev = 0; return hipSuccess; }

}  // namespace rec

// the host side of a kernel registers itself with the runtime when the program starts: nothing to register here (the program is linked
// without device code, -Wl,--unresolved-symbols=ignore-all for the missing code object)
extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kern, ...) ::rec::launch(kern, __VA_ARGS__)
#define hipFuncSetAttribute(fn, attr, value) ::rec::set_attr(fn)
#define hipGetDevice(dev) ::rec::get_device(dev)
#define hipGetLastError() hipSuccess

#include "mpk_rollout.hip"
#include "mpk_phase_fused.hip"
#include "mpk_traj_phase.hip"

namespace mpk {
// PhaseArgs and RowArgs are aggregate-initialised by launch_traj_rows, which leaves the padding behind init_time_shared (RowArgs: also
// behind B, its last member) to the stack: not part of what a kernel reads, zeroed before the bytes are hashed (found by
// argument-dependent lookup from rec::launch)
template <class A>
static void arg_bytes_no_padding(const A& a, size_t end) {
    A b;
    std::memcpy(&b, &a, sizeof(b));
    constexpr size_t from = offsetof(A, init_time_shared) + sizeof(float), to = offsetof(A, pos);
    std::memset(reinterpret_cast<char*>(&b) + from, 0, to - from);
    std::memset(reinterpret_cast<char*>(&b) + end, 0, sizeof(A) - end);
    rec::arg_bytes(reinterpret_cast<const unsigned char(&)[sizeof(A)]>(b));
}
static void arg_bytes(const PhaseArgs& a) { arg_bytes_no_padding(a, offsetof(PhaseArgs, h_pad) + sizeof(int)); }
static void arg_bytes(const RowArgs& a) { arg_bytes_no_padding(a, offsetof(RowArgs, B) + sizeof(int)); }
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace mpk

using namespace mpk;

namespace {

// made-up device addresses (never dereferenced): 16-byte aligned, `off` bytes past that on request
template <typename T>
T* fake(int slot, int off = 0) { return reinterpret_cast<T*>((uintptr_t)0x10000000u * (unsigned)(slot + 1) + (unsigned)off); }

struct Opt { std::string name; Tuning t; };

void alone(std::vector<Opt>& v, const char* key, int Tuning::*f, std::vector<int> vals) {
    for (int x : vals) { Opt o{std::string(key) + "=" + std::to_string(x), Tuning()}; o.t.*f = x; v.push_back(o); }
}
std::vector<int> range(int lo, int hi) { std::vector<int> r; for (int i = lo; i <= hi; ++i) r.push_back(i); return r; }

std::vector<Opt> rollout_options() {
    std::vector<Opt> v{{"default", Tuning()}};
    alone(v, "pd_quad", &Tuning::pd_quad, range(0, 3));
    alone(v, "pd_pipe", &Tuning::pd_pipe, range(0, 1));
    alone(v, "pd_simple", &Tuning::pd_simple, range(0, 1));
    alone(v, "pd_generic", &Tuning::pd_generic, range(0, 1));
    alone(v, "pd_helper", &Tuning::pd_helper, range(0, 1));
    alone(v, "write_through", &Tuning::write_through, range(0, 1));
    alone(v, "phase_waves", &Tuning::phase_waves, {0, 1, 4, 8});
    for (int quad : {0, 2, 3})
        for (int pipe : {0, 1}) {
            Opt o{"pd_quad=" + std::to_string(quad) + ",pd_pipe=" + std::to_string(pipe) + ",pd_helper=1,pd_generic=" + std::to_string(pipe), Tuning()};
            o.t.pd_quad = quad; o.t.pd_pipe = pipe; o.t.pd_helper = 1; o.t.pd_generic = pipe;
            v.push_back(o);
        }
    return v;
}

std::vector<Opt> phase_options() {
    std::vector<Opt> v{{"default", Tuning()}};
    alone(v, "phase", &Tuning::phase, range(0, 1));
    alone(v, "phase_chunk", &Tuning::phase_chunk, range(1, 16));
    alone(v, "phase_flat", &Tuning::phase_flat, range(0, 1));
    alone(v, "phase_table", &Tuning::phase_table, range(0, 1));
    alone(v, "phase_pipe", &Tuning::phase_pipe, range(0, 1));
    alone(v, "phase_split", &Tuning::phase_split, range(1, 8));
    alone(v, "phase_waves", &Tuning::phase_waves, {0, 1, 4, 8, 16});
    alone(v, "tiles_wpb", &Tuning::tiles_wpb, {1, 2, 4, 8});
    alone(v, "pipe", &Tuning::pipe, range(0, 1));
    alone(v, "pd_generic", &Tuning::pd_generic, range(0, 1));
    alone(v, "write_through", &Tuning::write_through, range(0, 1));
    for (int flat : {0, 1})
        for (int table : {0, 1})
            for (int chunk : {2, 8}) {
                Opt o{"phase_flat=" + std::to_string(flat) + ",phase_table=" + std::to_string(table) + ",phase_chunk=" + std::to_string(chunk) +
                          ",pd_generic=" + std::to_string(flat) + ",phase_pipe=" + std::to_string(table), Tuning()};
                o.t.phase_flat = flat; o.t.phase_table = table; o.t.phase_chunk = chunk; o.t.pd_generic = flat; o.t.phase_pipe = table;
                v.push_back(o);
            }
    return v;
}

const int kB[] = {1, 2, 3, 15, 16, 17, 64, 255, 256, 1024, 2048, 3071, 3072, 3073, 4096, 5119, 5120, 5121, 6144, 8191, 8192, 8193,
                  10239, 10240, 10241, 12287, 12288, 12289, 14336, 16384, 24575, 24576, 32768, 65536, 131072, 262144, 524288, 1048576};
const int kBQuick[] = {1, 17, 1024, 5120, 12288, 65536, 1048576};
const int kCU[] = {256, 8};

struct Sums {
    std::map<std::string, long> names, exits;
    long cases = 0;
};

void begin_case() { g_err.clear(); rec::g_text.clear(); }

// one case's record: return code, error text, kernel name, then what was raised and launched
unsigned long long finish(int rc, const char* name, Sums& s, std::string* text) {
    unsigned long long h = rec::fnv(&rc, sizeof(rc));
    h = rec::fnv(g_err.data(), g_err.size(), h);
    h = rec::fnv(name, std::strlen(name), h);
    h = rec::fnv(rec::g_text.data(), rec::g_text.size(), h);
    ++s.cases;
    if (rc == MPK_OK) ++s.names[name[0] ? name : "(none)"];
    else ++s.exits["rc=" + std::to_string(rc) + " err='" + g_err + "' name=" + (name[0] ? name : "unset")];
    if (text) *text = "rc=" + std::to_string(rc) + " err='" + g_err + "' name='" + name + "'" + rec::g_text;
    return h;
}

RolloutDev make_rc(int ctrl, int plant, int D) {
    RolloutDev rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.controller_type = ctrl; rc.plant_type = plant; rc.dt = 0.02;
    for (int d = 0; d < D && d < kMaxDofArgs; ++d) { rc.pg[d] = 1.0 + d; rc.dg[d] = 0.1 * (d + 1); rc.lo[d] = -1.0 - d; rc.hi[d] = 1.0 + 0.5 * d; }
    return rc;
}

// ---- rollouts: k = ((((ctrl * 2 + plant) * 2 + reward) * 2 + actions) * 2 + n_steps) * 3 + alignment (0 all 16-byte aligned, 1 inputs 4 bytes
// off, 2 actions 4 bytes off)
const int kRollKinds = 3 * 2 * 2 * 2 * 2 * 3;
unsigned long long rollout_case(int D, int T, const Tuning& tune, int B, int k, Sums& s, std::string* text) {
    const int al = k % 3, nst = k / 3 % 2, act = k / 6 % 2, rwd = k / 12 % 2, plant = k / 24 % 2, ctrl = k / 48;
    const RolloutDev rc = make_rc(ctrl, plant, D);
    const int io = al == 1 ? 4 : 0, ao = al == 2 ? 4 : 0;
    begin_case();
    int r;
    if (rwd)
        r = launch_reacher_rollout(rc, D, fake<float>(1, io), fake<float>(2, io), fake<double>(3), fake<double>(4), nst ? fake<int32_t>(5) : nullptr,
                                   nst ? fake<int32_t>(6) : nullptr, fake<double>(7), 190, act ? fake<float>(8, ao) : nullptr, fake<double>(9), B, T,
                                   nullptr, tune, fake<int>(10));
    else
        r = launch_pd_rollout(rc, D, fake<float>(1, io), fake<float>(2, io), fake<double>(3), fake<double>(4), nst ? fake<int32_t>(5) : nullptr,
                              act ? fake<float>(8, ao) : nullptr, B, T, nullptr, tune, fake<int>(10));
    return finish(r, "", s, text);
}

// ---- learned phase.  need: contraction columns (promp KT, dmp KT + 3, prodmp nb + 3); variant 0 fixed tau / delay, 1 both learned,
// 2 the handle's row table missing
const char* const kMpName[] = {"promp", "dmp", "prodmp"};
DevCfg make_cfg(int mp, int D, int T, int need, int variant) {
    DevCfg c;
    std::memset(&c, 0, sizeof(c));
    c.mp_type = mp;
    c.D = D; c.T = T;
    c.nb = mp == MPK_MP_PROMP ? need : need - 3;
    c.KT = mp == MPK_MP_PRODMP ? c.nb + 3 : c.nb;
    c.KP = (c.KT + 3) / 4 * 4;
    c.n_total = c.nb;
    c.Kloc = c.nb + (mp == MPK_MP_PROMP ? 0 : 1);
    c.learn_tau = c.learn_delay = variant == 1;
    c.off = c.learn_tau + c.learn_delay;
    c.P = D * c.Kloc + c.off;
    c.tau = 1.5f; c.delay = 0.0f; c.tau_lo = 0.5f; c.tau_hi = 3.0f; c.delay_lo = 0.0f; c.delay_hi = 0.25f;
    c.t_last = 0.02f * T;
    c.n_pc = 2 * T + 1; c.len_factor = 2; c.scaled_dt = 0.02f / 1.5f;
    c.tab = fake<double>(20); c.base_times = fake<float>(22);
    const int KS = need <= 8 ? 8 : 16;
    if (variant != 2) {
        c.rows32 = fake<float>(21);
        c.rows32_stride = mp == MPK_MP_PRODMP ? 2 * KS + 4 : (mp == MPK_MP_DMP ? 8 : 0);
    }
    return c;
}

// fused: kind 0 frozen-state actions, 1 closed loop, 2 + replanning state, 3 + gate, 4 lean (no outputs), 5 a gate on the static plant;
// k = ((controller * 6 + kind) * 2 + alignment) * 2 + init_time (0 / 0.3)
const int kFusedKinds = 3 * 6 * 2 * 2;
unsigned long long fused_case(const DevCfg& c, const Tuning& tune, int B, int cu, int k, Sums& s, std::string* text) {
    const int it = k % 2, al = k / 2 % 2, kind = k / 4 % 6, ctrl = k / 24;
    const bool closed = kind >= 1 && kind <= 4, rpl = kind == 2 || kind == 3, gated = kind == 3 || kind == 5, lean = kind == 4;
    const int oo = al ? 4 : 0;
    const RolloutDev rc = make_rc(ctrl, closed ? MPK_PLANT_DOUBLE_INTEGRATOR : MPK_PLANT_STATIC, c.D);
    ReplanDev rp;
    rp.traj_steps = fake<int32_t>(30); rp.plan_steps = fake<int32_t>(31); rp.done = fake<uint8_t>(32); rp.seg_len = fake<int32_t>(33);
    rp.cond_pos = fake<float>(34); rp.cond_vel = fake<float>(35); rp.every = 25; rp.max_planning_times = 4; rp.horizon = c.T;
    GateDev gd;
    for (int d = 0; d < kMaxD; ++d) { gd.lo[d] = -2.0 - 0.1 * d; gd.hi[d] = 2.0 + 0.3 * d; }
    gd.valid = fake<uint8_t>(40); gd.penalty = fake<double>(41);
    if (it) { gd.check_td = 1; gd.tau_b[0] = 0.5; gd.tau_b[1] = 3.0; gd.delay_b[1] = 0.25; gd.raw_params = fake<float>(42); }
    const char* name = "";
    begin_case();
    float* const pos = lean ? nullptr : fake<float>(4, oo);
    float* const vel = lean ? nullptr : fake<float>(5, oo);
    float* const actions = lean ? nullptr : fake<float>(6, oo);
    const int32_t* const n_steps = closed && !rpl ? fake<int32_t>(11) : nullptr;
    double* const ret = lean ? fake<double>(12) : nullptr;
    int32_t* const seg_out = lean ? fake<int32_t>(13) : nullptr;
#ifdef LAUNCH_POSITIONAL_CALLS
    const int r = launch_phase_fused(c, fake<float>(1), fake<float>(2), fake<float>(3), it ? 0.3f : 0.0f, pos, vel, actions, rc, fake<double>(9),
                                     fake<double>(10), n_steps, rpl ? &rp : nullptr, gated ? &gd : nullptr, ret, seg_out, fake<int32_t>(14), B, cu,
                                     nullptr, &name, tune, fake<int>(15));
#else
    TrajRequest req;
    req.params = fake<float>(1); req.init_pos = fake<float>(2); req.init_vel = fake<float>(3); req.init_time_shared = it ? 0.3f : 0.0f;
    req.pos = pos; req.vel = vel; req.actions = actions; req.rc = &rc; req.n_steps = n_steps;
    // (the state the kernel reads: the closed loop's plant state, else the frozen one)
    if (closed) { req.q_state = fake<double>(9); req.qd_state = fake<double>(10); }
    else { req.c_pos = fake<double>(9); req.c_vel = fake<double>(10); }
    req.rp = rpl ? &rp : nullptr; req.gate = gated ? &gd : nullptr; req.ep.ret = ret; req.ep.seg_out = seg_out; req.B = B;
    LaunchSite at;
    at.num_cu = cu; at.tune = tune; at.kernel_name = &name; at.fault = fake<int>(15); at.range_flag = fake<int32_t>(14);
    const int r = launch_phase_fused(c, req, at);
#endif
    return finish(r, name, s, text);
}

// rows: k = alignment * 3 + init_time (0 shared 0, 1 shared 0.3, 2 per episode)
const int kRowsKinds = 2 * 3;
unsigned long long rows_case(const DevCfg& c, const Tuning& tune, int B, int cu, int k, Sums& s, std::string* text) {
    const int it = k % 3, oo = k / 3 ? 4 : 0;
    const char* name = "";
    begin_case();
#ifdef LAUNCH_POSITIONAL_CALLS
    const int r = launch_traj_rows(c, fake<float>(1), fake<float>(2), fake<float>(3), it == 2 ? fake<float>(16) : nullptr, it == 1 ? 0.3f : 0.0f,
                                   fake<float>(4, oo), fake<float>(5, oo), fake<int32_t>(14), B, cu, nullptr, &name, tune);
#else
    TrajRequest req;
    req.params = fake<float>(1); req.init_pos = fake<float>(2); req.init_vel = fake<float>(3);
    req.init_time = it == 2 ? fake<float>(16) : nullptr; req.init_time_shared = it == 1 ? 0.3f : 0.0f;
    req.pos = fake<float>(4, oo); req.vel = fake<float>(5, oo); req.B = B;
    LaunchSite at;
    at.num_cu = cu; at.tune = tune; at.kernel_name = &name; at.range_flag = fake<int32_t>(14);
    const int r = launch_traj_rows(c, req, at);
#endif
    // where launch_traj_phase declined (the launch went on to k_traj_rows or its LDS check): which of its exits, by the shape
    if (tune.phase != 0 && !(c.mp_type == MPK_MP_PROMP && c.T < 2) && std::strncmp(name, "k_traj_phase", 12) != 0) {
        const bool prodmp = c.mp_type == MPK_MP_PRODMP;
        const int need = prodmp ? c.nb + 3 : c.KT + (c.mp_type == MPK_MP_DMP ? 3 : 0);
        const int KS = need <= 4 && c.mp_type == MPK_MP_PROMP ? 4 : (need <= 8 ? 8 : 16);
        ++s.exits[std::string("k_traj_phase declined: ") + (need > 16 || c.D > 64 ? "need > 16" : c.D * KS > 256 ? "D * KS > 256" :
                  prodmp && (!c.rows32 || c.rows32_stride != 2 * KS + 4) ? "rows32 missing" : "LDS overflow")];
    }
    return finish(r, name, s, text);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: launch_rec <rollout | fused | rows> <shard 0..7 | all> [--quick | --dump KEY]\n"); return 2; }
    const std::string unit = argv[1];
    const int shard = std::strcmp(argv[2], "all") != 0 ? std::atoi(argv[2]) : -1;
    const bool quick = argc > 3 && std::strcmp(argv[3], "--quick") == 0;
    const char* dump = argc > 4 && std::strcmp(argv[3], "--dump") == 0 ? argv[4] : nullptr;
    std::vector<int> Bs = quick ? std::vector<int>(std::begin(kBQuick), std::end(kBQuick)) : std::vector<int>(std::begin(kB), std::end(kB));
    Sums s;
    // one block: every batch size, CU count and call kind of a (shape, option)
    auto block = [&](const std::string& key, int kinds, bool with_cu, auto&& one) {
        if (dump && key != dump) return;
        unsigned long long h = 1469598103934665603ull;
        long n = 0;
        std::string text;
        for (int B : Bs) for (int cu : kCU) {
            if (!with_cu && cu != kCU[0]) continue;
            for (int k = 0; k < kinds; ++k) {
                const unsigned long long hc = one(B, cu, k, dump ? &text : nullptr);
                h = rec::fnv(&hc, sizeof(hc), h);
                ++n;
                if (dump) std::printf("B=%d cu=%d kind=%d | %s\n", B, cu, k, text.c_str());
            }
        }
        if (!dump) std::printf("BLOCK\t%s\t%ld\t%016llx\n", key.c_str(), n, h);
    };
    if (unit == "rollout") {
        const int kD[] = {1, 2, 3, 5, 7, 8, 16, 17}, kT[] = {1, 2, 16, 17, 25, 100, 200, 1000};
        const std::vector<Opt> opts = rollout_options();
        for (int di = 0; di < 8; ++di) {
            if (shard >= 0 && di != shard) continue;
            for (int T : kT) for (const Opt& o : opts) {
                if (quick && T != 2 && T != 100) continue;
                const int D = kD[di];
                block("rollout D=" + std::to_string(D) + " T=" + std::to_string(T) + " " + o.name, kRollKinds, false,
                      [&](int B, int, int k, std::string* text) { return rollout_case(D, T, o.t, B, k, s, text); });
            }
        }
    } else {
        // (T = 40000: the launchers' own LDS overflow exits; T = 20000: the dmp pipeline exit above 64 KB of LDS, where 7 DoF and "pd_generic"
        // meet; both with the default options and "pd_generic" only)
        const int kD[] = {1, 2, 5, 7, 8, 16, 17, 64}, kT[] = {1, 2, 17, 49, 100, 300, 350, 1000, 20000, 40000}, kNeed[] = {4, 8, 9, 16, 17};
        const bool fused = unit == "fused";
        const std::vector<Opt> opts = phase_options();
        for (int di = 0; di < 8; ++di) {
            if (shard >= 0 && di != shard) continue;
            for (int mp = 0; mp < 3; ++mp) for (int T : kT) for (int need : kNeed) for (int variant = 0; variant < 3; ++variant) {
                if (quick && T != 2 && T != 100 && T < 20000) continue;
                if (mp != MPK_MP_PROMP && need - 3 < 1) continue;
                const int D = kD[di];
                const DevCfg c = make_cfg(mp, D, T, need, variant);
                for (const Opt& o : opts) {
                    if (variant == 2 && &o != &opts[0]) continue;
                    if (T >= 20000 && &o != &opts[0] && o.name.compare(0, 10, "pd_generic") != 0) continue;
                    const std::string key = unit + " " + kMpName[mp] + " D=" + std::to_string(D) + " T=" + std::to_string(T) + " need=" + std::to_string(need) +
                                            " variant=" + std::to_string(variant) + " " + o.name;
                    if (fused) block(key, kFusedKinds, true, [&](int B, int cu, int k, std::string* text) { return fused_case(c, o.t, B, cu, k, s, text); });
                    else block(key, kRowsKinds, true, [&](int B, int cu, int k, std::string* text) { return rows_case(c, o.t, B, cu, k, s, text); });
                }
            }
        }
    }
    if (!dump) {
        for (const auto& kv : s.names) std::printf("NAME\t%s\t%ld\n", kv.first.c_str(), kv.second);
        for (const auto& kv : s.exits) std::printf("EXIT\t%s\t%ld\n", kv.first.c_str(), kv.second);
        for (const auto& kv : rec::g_syms) std::printf("SYM\t%s\t%ld\n", kv.first.c_str(), kv.second);
        std::printf("CASES\t%ld\n", s.cases);
    }
    return 0;
}
