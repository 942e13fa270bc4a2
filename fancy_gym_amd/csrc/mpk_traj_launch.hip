// k_build_shared (phase / exponential-kernel evaluation for a phase all episodes share), plan_traj_shared: the rule that picks a
// shared-phase trajectory kernel family, its work decomposition and its store policy for a launch, as a value (TrajRoute,
// mpk_traj_route.h), and launch_traj_shared: plan + launch.  plan_episode_return / launch_episode_return: the same for k_episode_return.
#include <cstdio>

#include "mpk_tile.h"
#include "mpk_traj_quad.h"   // kQuadImg, kPipeGroups: the LDS budgets the rule checks
#include "mpk_traj_pipe.h"
#include "mpk_traj_stream.h" // kChunkGroups
#include "mpk_traj_ring.h"   // kRingThreads, kRingSyncInts
#include "mpk_traj_route.h"

namespace mpk {

// a shape only k_traj_wide can take (more than kMaxKP columns, or more than kMaxD DoF): that kernel reads the position rows
// (prodmp: + velocity rows) of the k-major table and nothing else, so such a handle's slots hold just those -- no
// finite-difference operand rows, no step-major copy (a sixth of the full promp table: ~1.7 MB instead of 10 MB per slot at
// K = 1000, T = 200)
bool shared_tables_lean(const DevCfg& c) { return c.KP > kMaxKP || c.D > kMaxD; }

size_t shared_tables_floats(const DevCfg& c, int* TS, int* n_out) {
    const int TP = (c.T + 15) / 16 * 16;
    const int ts = ((TP + 15) / 32) * 32 + 16;  // TS % 32 == 16: the two k rows of a 32-lane LDS read hit disjoint banks
    const bool lean = shared_tables_lean(c);
    const int no = c.mp_type == MPK_MP_PRODMP ? 2 : (c.mp_type == MPK_MP_PROMP && !lean ? 3 : 1);
    *TS = ts;
    *n_out = no;
    // the k-major table A [n_out][KP][TS] (MFMA fragment loads) followed by its step-major copy At [TS][n_out * KP]
    // (one contiguous row per time step: the serial role of k_traj_split reads it with scalar loads)
    return (lean ? 1 : 2) * (size_t)no * c.KP * ts;
}

// ------------------------------------------------------------------------------------------------------------
// k_build_shared: one block; A[(j*KP + k)*TS + t], aux[t]
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_build_shared(const DevCfg c, const float init_time, float* __restrict__ A,
                                                      float* __restrict__ aux, const int TS, const int n_out, const int lean,
                                                      int32_t* __restrict__ idx_out, int32_t* __restrict__ flag) {
    const int tid = threadIdx.x, T = c.T, KP = c.KP;
    for (int i = tid; i < n_out * KP * TS; i += 256) A[i] = 0.0f;
    for (int i = tid; i < TS; i += 256) aux[i] = 0.0f;
    __syncthreads();
    if (c.dmp_resp) {
        // DMP with a phase all episodes share, as a CONTRACTION (round 5).  The explicit Euler recurrence of the reference's DMP
        // (the CPU restatement's dmp_trajectory: a = alpha (beta (g - y) - z) + f; z += ds a; y += ds z; vel = z / tau) is
        // linear in (w, g, y_b, v_b): pos[t] = sum_k R_pos[t, k] x_k with x = (w_1 .. w_nb, g, y_b, v_b), and R the response of THE
        // SAME Euler map -- same fp32 step sizes ds, same order of operations -- to the unit inputs, run here once per (init_time, T)
        // in float64 and rounded once to fp32.  Superposition of explicit Euler, not the ODE's analytic solution: first-order
        // convergence in dt stays what the reference's integrator gives (tests/test_gpu_ode.py).  Columns as ProDMP's: weights, goal,
        // y_b, v_b -- the two-output matrix-core kernels run unchanged (and with them fused actions and the closed loop).  The host
        // takes this route only where the Euler map is stable (alpha ds < 1: mpk_host.cpp dmp_response_ok), i.e. |R| = O(1).
        const int nb = c.nb;
        // (1) forcing rows phi_k(x) x weights_scale as the serial kernels contract them (fp32), aux = fp32 step sizes
        for (int t = tid; t < T; t += 256) {
            const float time = c.base_times[t] + init_time;
            const double x = phase_f64(c, time, c.tau, c.delay, ExpLiteral());
            rbf_cols(c, x, x * (double)c.ws, A + t, TS);
            if (t < T - 1) {
                const float s0 = scaled_time(time, c.delay, c.tau);
                const float s1 = scaled_time(c.base_times[t + 1] + init_time, c.delay, c.tau);
                aux[t] = s1 - s0;
            }
        }
        __syncthreads();
        // (2) one thread per unit input runs the T - 1 steps (a forcing value is read before its slot takes the response)
        if (tid < nb + 3) {
            const int k = tid;
            const double al = (double)c.dmp_alpha, be = (double)c.dmp_beta, tau = (double)c.tau, itau = div_pos(1.0, (double)c.tau);
            const double G = k == nb ? (double)c.gs : 0.0;
            double y = k == nb + 1 ? 1.0 : 0.0, z = k == nb + 2 ? tau : 0.0;      // z_0 = tau v_b
            // sixteen steps per trip: their forcing values and step sizes are read TOGETHER, in front of the trip's stores (the response
            // takes the forcing value's slot, so the compiler cannot hoist a load over the stores before it: step by step the loop was T
            // dependent round trips to the table -- hundreds of us at T = 200 whenever a plan brings a new init_time; review of round 5)
            constexpr int U = 16;
            float fn[U], dn[U];
            auto fetch = [&](const int t0) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = t0 + u < T ? t0 + u : T - 1;
                    fn[u] = k < nb ? A[(size_t)k * TS + t] : 0.0f;
                    dn[u] = aux[t];
                }
            };
            fetch(0);
            for (int t0 = 0; t0 < T; t0 += U) {
                float fv[U], dv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) { fv[u] = fn[u]; dv[u] = dn[u]; }
                if (t0 + U < T) fetch(t0 + U);           // the next trip's values: in flight while this trip's steps run
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = t0 + u;
                    if (t < T) {
                        A[(size_t)(0 * KP + k) * TS + t] = (float)y;
                        A[(size_t)(1 * KP + k) * TS + t] = (float)(z * itau);
                        if (t < T - 1) {
                            const double acc = al * (be * (G - y) - z) + (double)fv[u];
                            z = z + (double)dv[u] * acc;
                            y = y + (double)dv[u] * z;
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < TS; i += 256) aux[i] = 0.0f;
    } else if (c.mp_type == MPK_MP_PRODMP) {
        const float sb = scaled_time(init_time, c.delay, c.tau);
        const int idxb = min(prodmp_index(sb, c.scaled_dt), c.n_pc - 1);
        ProdmpBC bc;
        prodmp_bc(c, idxb, bc);
        if (idx_out && tid == 0) idx_out[T] = idxb;
        for (int t = tid; t < T; t += 256) {
            const float time = c.base_times[t] + init_time;
            const float s = scaled_time(time, c.delay, c.tau);
            if (s > (float)c.len_factor) atomicOr(flag, 1);
            const int idx = min(prodmp_index(s, c.scaled_dt), c.n_pc - 1);
            if (idx_out) idx_out[t] = idx;
            double xi[4];
            prodmp_xi(c, bc, idx, xi);
            for (int k = 0; k < c.KT; ++k) {
                float h, hv;
                prodmp_col(c, bc, idx, xi, k, (double)c.tau, div_pos(1.0, (double)c.tau), &h, &hv);
                A[(size_t)(0 * KP + k) * TS + t] = h;
                A[(size_t)(1 * KP + k) * TS + t] = hv;
            }
        }
    } else if (c.mp_type == MPK_MP_PROMP) {
        for (int t = tid; t < T; t += 256) {
            const float time = c.base_times[t] + init_time;
            const double x = phase_f64(c, time, c.tau, c.delay, ExpLiteral());
            rbf_cols(c, x, (double)c.ws, A + t, TS);
            if (c.KT > c.nb) A[(size_t)c.nb * TS + t] = 1.0f;  // zero-padded family: + init_pos
        }
        __syncthreads();
        // velocity = forward difference: rows (t+1, t), last row repeats (T-1, T-2)
        for (int t = tid; t < T; t += 256) {
            const int th = t < T - 1 ? t + 1 : T - 1, tl = t < T - 1 ? t : T - 2;
            for (int k = 0; k < c.KT && !lean; ++k) {
                A[(size_t)(1 * KP + k) * TS + t] = A[(size_t)k * TS + th];
                A[(size_t)(2 * KP + k) * TS + t] = A[(size_t)k * TS + tl];
            }
            // reciprocal of the fp32 time step (one IEEE divide per row here instead of one per output element later)
            aux[t] = 1.0f / ((c.base_times[th] + init_time) - (c.base_times[tl] + init_time));
        }
    } else {  // DMP: forcing rows phi*x, aux = diff of the fp32 scaled times
        for (int t = tid; t < T; t += 256) {
            const float time = c.base_times[t] + init_time;
            const double x = phase_f64(c, time, c.tau, c.delay, ExpLiteral());
            rbf_cols(c, x, x * (double)c.ws, A + t, TS);
            if (t < T - 1) {
                const float s0 = scaled_time(time, c.delay, c.tau);
                const float s1 = scaled_time(c.base_times[t + 1] + init_time, c.delay, c.tau);
                aux[t] = s1 - s0;
            }
        }
    }
    // step-major copy behind the k-major table: one contiguous row per step; with two outputs (prodmp) the row is
    // interleaved [pos_0 vel_0 pos_1 vel_1 ..] -- the operand pairs of the packed fp32 FMA the serial role contracts with
    __syncthreads();
    if (lean) return;
    const int RS = n_out * KP;
    float* At = A + (size_t)RS * TS;
    for (int i = tid; i < RS * TS; i += 256) {
        const int t = i / RS, e = i - t * RS;
        const int jk = n_out == 2 ? (e & 1) * KP + (e >> 1) : e;
        At[i] = A[(size_t)jk * TS + t];
    }
}

#ifndef MPK_DEVICE_ONLY
int launch_build_shared(const DevCfg& c, float init_time, const SharedTables& st, int32_t* idx_out,
                        int32_t* range_flag, void* stream) {
    if (c.mp_type == MPK_MP_PROMP && c.T < 2) {
        set_error("promp needs at least two time steps for the finite-difference velocity");
        return MPK_EINVAL;
    }
    hipLaunchKernelGGL(k_build_shared, dim3(1), dim3(256), 0, (hipStream_t)stream, c, init_time, st.A, st.aux, st.TS,
                       st.n_out, shared_tables_lean(c) ? 1 : 0, idx_out, range_flag);
    MPK_LAUNCH_CHECK();
    return MPK_OK;
}
#endif  // MPK_DEVICE_ONLY

#ifndef MPK_DEVICE_ONLY
static void fill_gate_args(const GateDev* gate, const float* params, int D, TrajArgs& ta, ActArgs& aa) {
    ta.gate_valid = nullptr; ta.gate_penalty = nullptr; ta.gate_raw = nullptr; ta.gate_check_td = 0;
    ta.gate_tb[0] = ta.gate_tb[1] = ta.gate_db[0] = ta.gate_db[1] = 0.0;
    if (!gate) return;
    ta.gate_valid = gate->valid; ta.gate_penalty = gate->penalty;
    ta.gate_raw = gate->raw_params ? gate->raw_params : params;
    ta.gate_check_td = gate->check_td;
    ta.gate_tb[0] = gate->tau_b[0]; ta.gate_tb[1] = gate->tau_b[1];
    ta.gate_db[0] = gate->delay_b[0]; ta.gate_db[1] = gate->delay_b[1];
    for (int d = 0; d < D; ++d) {
        aa.glo[d] = gate->lo[d]; aa.ghi[d] = gate->hi[d];
        aa.glo32[d] = f32_at_least(gate->lo[d]); aa.ghi32[d] = f32_at_most(gate->hi[d]);
    }
}

// what plan_traj_shared and plan_episode_return both copy from the request: configuration, tables, inputs, the batch and its episode
// groups, plant and replanning state, the controller's gains and limits (gains: a controller runs), the gate
static void fill_request_args(const DevCfg& c, const SharedTables& st, const TrajRequest& q, bool gains, TrajArgs& ta, ActArgs& aa) {
    ta.wpb = 4; ta.ring_parts = 1;
    if (q.rp) ta.rp = *q.rp;
    ta.q_state = q.q_state; ta.qd_state = q.qd_state; ta.n_steps = q.n_steps; ta.plant_dt = q.rc ? q.rc->dt : 0.0;
    ta.c = c; ta.A = st.A; ta.aux = st.aux; ta.TS = st.TS;
    ta.params = q.params; ta.init_pos = q.init_pos; ta.init_vel = q.init_vel;
    ta.B = q.B;
    int sh = 0;
    while ((1 << sh) < c.D) ++sh;  // DP = next power of two >= D (<= 16)
    ta.sh = sh;
    const int NTW = 16 >> sh;
    ta.G = (q.B + NTW - 1) / NTW;
    if (gains)
        for (int d = 0; d < c.D; ++d) { aa.pg[d] = q.rc->pg[d]; aa.dg[d] = q.rc->dg[d]; aa.lo[d] = q.rc->lo[d]; aa.hi[d] = q.rc->hi[d]; }
    fill_gate_args(q.gate, q.params, c.D, ta, aa);
}

// mpk_episode_return: plan + controller + plant + reward + aggregation of a `verbose < 2` step in one launch (k_episode_return).
// MPK_ENOTIMPL where the tables do not fit beside the images (long horizons): the caller's separate launches take those.
// The geometry choice; no HIP call, no allocation.  (A route's name is set as soon as its kernel is known, also where the plan then declines.)
int plan_episode_return(const DevCfg& c, const SharedTables& st, const TrajRequest& q, int num_cu, const Tuning& tune, TrajArgs& ta,
                        ActArgs& aa, EpArgs& ea, EpRoute& r) {
    const int reward_type = q.ep.reward;
    fill_request_args(c, st, q, true, ta, aa);
    const int NTW = 16 >> ta.sh;
    const int SEG = 16 * c.D;
    ta.pitch = SEG; ta.cps = SEG / 4 > 0 ? SEG / 4 : 1; ta.inv_cps = 65536u / (unsigned)ta.cps + 1u; ta.vec_ok = 1;      // (never the shifted staging image)
    ea.ret = q.ep.ret; ea.goal = q.ep.goal; ea.step0 = q.ep.step0; ea.seg_out = q.ep.seg_out; ea.steps_before_reward = q.ep.steps_before_reward;
    ea.agg = q.ep.agg;
    ea.km = c.KP / 4;
    const size_t table_bytes = ((size_t)st.n_out * c.KP * st.TS + st.TS) * sizeof(float);
    // groups per wave: four while that still gives every SIMD a wave (the chain is latency bound: more lanes per instruction),
    // else two, else one ("quad" 2 / 3 / 4 force four / two / one)
    const long simds = (long)num_cu * 4;
    int nq = ta.G >= 4 * simds ? 4 : (ta.G >= 2 * simds ? 2 : 1);
    if (tune.quad == 2) nq = 4; else if (tune.quad == 3) nq = 2; else if (tune.quad == 4) nq = 1;
    while (reward_type && nq > 1 && nq * NTW > 4 * kEpMaxPass) nq >>= 1;      // the reward pass keeps two accumulators per lane
    const size_t img = reward_type ? kEpImg : kEpImgPlain;
    auto lds_of = [&](int n, int w) { return table_bytes + ((size_t)w * n * img + (size_t)w * kEpSlots * kEpSlotInts) * sizeof(float); };
    while (nq > 1 && lds_of(nq, 4) > kLdsPerCu) nq >>= 1;
    if (lds_of(nq, 4) > kLdsPerCu || (reward_type && nq * NTW > 4 * kEpMaxPass)) { set_error("trajectory too long for the episode kernel's LDS budget"); return MPK_ENOTIMPL; }
    // eight waves per workgroup where that puts more waves on a CU than four-wave workgroups do (they share one table copy)
    const long units = ((long)ta.G + nq - 1) / nq;
    const long w4 = (long)(kLdsPerCu / lds_of(nq, 4)) * 4, w8 = lds_of(nq, 8) <= kLdsPerCu ? (long)(kLdsPerCu / lds_of(nq, 8)) * 8 : 0;
    int wpb = w8 > w4 && units >= 8L * num_cu ? 8 : 4;
    if (tune.tiles_wpb == 4 || tune.tiles_wpb == 8) wpb = tune.tiles_wpb == 8 && w8 > 0 ? 8 : 4;     // ("tiles_wpb" 4 / 8: A/B runs, tests)
    ea.wpb = wpb;
    r.lds = lds_of(nq, wpb);
    const long per_cu = (long)(kLdsPerCu / r.lds) < 1 ? 1 : (long)(kLdsPerCu / r.lds);
    long blocks = (units + wpb - 1) / wpb;
    const long cap = (long)num_cu * (per_cu > 8 ? 8 : per_cu);
    if (blocks > cap) blocks = cap;
    if (blocks >= 8) blocks = (blocks + 7) / 8 * 8;
    r.blocks = (int)blocks;
    r.ct = q.rc->controller_type + 3; r.nq = nq; r.rwd = reward_type;
    const bool pd = c.mp_type == MPK_MP_PRODMP;
    r.name = reward_type ? (pd ? "k_episode_return<prodmp,reacher>" : "k_episode_return<promp,reacher>")
                         : (pd ? "k_episode_return<prodmp>" : "k_episode_return<promp>");
    if (c.mp_type == MPK_MP_DMP) { set_error("internal: the episode kernel takes promp / prodmp rows"); return MPK_EINVAL; }
    return MPK_OK;
}

int launch_episode_return(const DevCfg& c, const SharedTables& st, const TrajRequest& q, const LaunchSite& at) {
    TrajArgs ta{};
    ActArgs aa{};
    EpArgs ea{};
    EpRoute r{};
    const int rc_ = plan_episode_return(c, st, q, at.num_cu, at.tune, ta, aa, ea, r);
    if (r.name) *at.kernel_name = r.name;
    if (rc_ != MPK_OK) return rc_;
    return by_mp_type(c.mp_type, [&](auto mp) { return launch_episode_kernel<decltype(mp)::value>(ta, aa, ea, r, at.stream); });
}

// ------------------------------------------------------------------------------------------------------------
// The route of a shared-phase launch (trajectory, fused actions, closed-loop step, replanning step, gated step): plan_traj_shared
// asks the kernel families in their order of precedence; each family's function below either declines or fills the route and its
// part of TrajArgs.  Pure arithmetic on shapes, pointer alignment and options: no HIP call, no allocation.
// ------------------------------------------------------------------------------------------------------------
// what every family's rule reads, gathered once per launch
struct TrajFacts {
    const DevCfg& c;
    const Tuning& tune;
    int B, num_cu;
    bool dmp, closed, act, gated;
    bool ptr_ok;                 // output arrays 16-byte aligned
    bool in_ok;                  // input arrays 16-byte aligned (k_traj_stream's bulk staging)
    int NTW, NRT, TD, nst;       // episodes per group, row tiles, floats per trajectory, output arrays
    long max_waves;              // 8 waves per SIMD resident
    size_t table_bytes;
    size_t lds_pad;              // "lds_pad" in bytes: occupancy experiments (A/B runs)
    double out_bytes;
    int ov;                      // mpk_set_option "mapping"
    bool pipe, split;            // the closed loop's k_traj_pipe / (forced) k_traj_split take the launch
    bool serial;                 // serial-recurrence launch (DMP, closed loop) outside k_traj_split: episode-major or nothing
    bool episode_major;          // work decomposition where no ring / pipe / lane-quarter kernel takes the launch
    int flat_img;                // floats per (array, group) whole-trajectory image, rounded to float4
    size_t lds_flat;
    bool flat_ok, flat_takes_it;
    double stream_from;
    unsigned* ticket;
};

static int at_most(long n, long cap) { return (int)(n < cap ? n : cap); }

// wave-specialised store engine (k_traj_ring): ONE persistent workgroup per CU whose LDS holds the tables + a ring of NBUF
// batch buffers of M whole-trajectory group images; producer waves fill them (contraction + controller epilogue), store-engine
// waves write each batch's arrays as contiguous runs; batches are handed out in order from one device counter.  Open loop,
// promp / prodmp (the serial-recurrence variants need four groups per wave: mpk_traj_ring.hip).  Automatic once a launch writes more than kRingBytes (A/B
// measurements: profiles/r04_ring.md); mpk_set_option "ring": 0 off, 1 force; "ring_np" / "ring_ns" / "ring_m" /
// "ring_parts": producer waves, store-engine waves, groups per batch, waves per group.  A forced episode-major variant
// ("quad", "bulk", "flat" 1, "pipe" 1, "split" 1) wins over the automatic choice.
static bool plan_ring_open(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const Tuning& tune = f.tune;
    const bool forced_other = tune.flat == 1 || tune.bulk >= 0 || tune.quad >= 0 || tune.pipe == 1 || tune.split == 1 || f.ov == 1;
    // (trajectory-only launches that k_traj_flat takes -- two workgroups of whole-trajectory images per CU, see below -- stay there
    // up to kRingTrajBytes: round 5, cfg2's shape, us flat / ring: 65 536 episodes 68.8 / 80.4, 131 072: 134.7 / 149.3, 262 144:
    // 259.5 / 282.7, 524 288: 533.8 / 551.9, 1 048 576: 1 151 / 1 092.  With actions the ring stays ahead from kRingBytes on.)
    const bool want = tune.ring == 1 || (tune.ring < 0 && !forced_other && f.out_bytes > (f.flat_takes_it ? kRingTrajBytes : kRingBytes));
    int NS = tune.ring_ns > 0 ? tune.ring_ns : 2;
    int NP = tune.ring_np > 0 ? tune.ring_np : 8;
    if (NS > 8) NS = 8;
    if (NP + NS > kRingThreads / 64) NP = kRingThreads / 64 - NS;
    const size_t fixed = f.table_bytes + kRingSyncInts * sizeof(int);
    const int gimg = f.NTW * f.TD;                                // floats per (array, group) image, exactly
    auto buf_of = [&](int m) { return (size_t)f.nst * m * gimg * sizeof(float); };
    // groups per batch: as asked ("ring_m"), else the most (<= 4) that leave two batch buffers in the CU's LDS; a batch
    // must be a whole number of float4 per array (its runs are written as aligned 16-byte chunks)
    auto fits = [&](int m) { return fixed + 2 * buf_of(m) <= kLdsPerCu && ((long)m * gimg) % 4 == 0; };
    int M = tune.ring_m > 0 ? tune.ring_m : 4;
    while (M > 1 && !fits(M)) --M;
    if (!(f.ptr_ok && want && !f.closed && !f.dmp && tune.ring != 2 && fits(M))) return false;
    const size_t buf_bytes = buf_of(M);
    long nbuf = (long)((kLdsPerCu - fixed) / buf_bytes);
    if (nbuf * M > 32) nbuf = 32 / M;                             // 32 slots of sync counters
    if (nbuf > 3) nbuf = 3;
    // waves per group: with few slots (long horizons: one group's image fills a buffer) the producers share a group's
    // row tiles, so that all of them have work
    int P = tune.ring_parts > 0 ? tune.ring_parts : (int)((NP + nbuf * M - 1) / (nbuf * M));
    if (P > f.NRT) P = f.NRT;
    if (P > 8) P = 8;
    if (P < 1) P = 1;
    ta.flat_img = gimg;
    ta.ring_np = NP; ta.ring_ns = NS; ta.ring_m = M; ta.ring_nbuf = (int)nbuf; ta.ring_parts = P;
    // in-order dynamic batch assignment: tickets of TB batches from one counter word (~88 tickets / us at most: a
    // ticket must be worth well over 100 KB of output); zero at handle creation, zeroed again by the launch's last workgroup
    ta.ring_ctr = f.ticket;
    ta.ring_tb = (int)((kRingTicketBytes + buf_bytes - 1) / buf_bytes);
    const long batches = ((long)ta.G + M - 1) / M;
    {
        // ... but never so coarse that a workgroup sees fewer than ~16 tickets: wave 0 takes its first 3 - 4 tickets in ONE
        // atomic, so with tickets of five batches the first workgroups to start walked off with 15 - 20 batches each -- at
        // 12 288 episodes (6 batches per workgroup on average) a few dozen workgroups did all the work while the rest found
        // the counter past the end: THE ring's "fixed" 33 - 38 us below ~30 000 episodes (round 5, tools/ring_floor_probe.py:
        // no production + no stores 34 us with tickets, 8 us with static batches), and a coarse tail at 65 536
        const long fine = batches / (16L * (batches < (long)f.num_cu ? batches : (long)f.num_cu));
        if (tune.ring_tb > 0) ta.ring_tb = tune.ring_tb;
        else if ((long)ta.ring_tb > fine) ta.ring_tb = (int)fine;
    }
    if (ta.ring_tb < 1) ta.ring_tb = 1;
    // (the kernel keeps 2 + ceil(2 NP / (TB M P)) tickets in flight in 8 slots: a ticket covers at least NP / 2 work units)
    while (2 * ta.ring_tb * M * P < NP) ++ta.ring_tb;
    r.family = TrajFamily::RingOpen;
    r.lds = fixed + (size_t)nbuf * buf_bytes;
    r.blocks = at_most(batches, f.num_cu);
    return true;
}

// closed loop on the ring (k_traj_ring<.., closed>): producers + store engine for pos / vel, consumer waves for the recurrences
// (mpk_traj_ring.h).  LDS: tables + NBUF (pos | vel) batch buffers of four groups + one 4 KB action tile set per consumer.
static bool plan_ring_closed(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const DevCfg& c = f.c;
    const Tuning& tune = f.tune;
    if (!(f.closed && !f.gated && !f.dmp && f.act && f.ptr_ok && f.TD % 4 == 0 && (c.D == 5 || c.D == 7) && c.KP <= 8 && !f.split &&
          tune.ring != 0 && tune.ring != 2)) return false;
    const bool forced_other = tune.quad >= 0 || tune.pipe == 1 || tune.split == 1 || f.ov != 0 || tune.bulk >= 0;
    const bool want = tune.ring == 1 || (tune.ring < 0 && !forced_other && !f.pipe && f.out_bytes > kRingClosedBytes);
    // geometry by the sweep in profiles/r04_ring_closed.md: the fewer waves store, the better (one engine wave), production and
    // recurrences need eight and four waves to keep three batch buffers turning
    int NS = tune.ring_ns > 0 ? tune.ring_ns : 1;
    int NP = tune.ring_np > 0 ? tune.ring_np : 8;
    int NC = tune.ring_nc > 0 ? tune.ring_nc : 3;
    if (NS > 4) NS = 4;
    const int AW = (ta.ring_dbg & 8) ? 0 : 1;                            // "ring_dbg" 8: the consumers store their action tiles themselves
    if (NP + NS + NC * (1 + AW) > kRingThreadsClosed / 64) NP = kRingThreadsClosed / 64 - NS - NC * (1 + AW);
    int M = tune.ring_m > 0 && tune.ring_m < 4 ? tune.ring_m : 4;          // groups per batch = lane quarters of a consumer
    const int gimg = f.NTW * f.TD;
    const size_t fixed = f.table_bytes + kRingSyncInts * sizeof(int);
    const size_t stage = (size_t)NC * 4 * kStageStride * sizeof(float);
    // (longer horizons: fewer groups per batch, while that leaves at least two batch buffers)
    while (M > 1 && fixed + stage + 2 * (size_t)2 * M * gimg * sizeof(float) > kLdsPerCu) --M;
    const size_t buf_bytes = (size_t)2 * M * gimg * sizeof(float);
    long nbuf = fixed + stage < kLdsPerCu ? (long)((kLdsPerCu - fixed - stage) / buf_bytes) : 0;
    if (nbuf * M > 32) nbuf = 32 / M;
    if (nbuf > 4) nbuf = 4;
    // automatic only with four groups per batch (one per lane quarter of a consumer): a 200-step horizon leaves room for two, and
    // the ring then loses to the lane-quarter kernels (round 5, cfg3's shape closed loop, us ring / duo: 32 768 episodes 192 / 124,
    // 65 536: 368 / 280, 131 072: 722 / 522 -- tools/dmp_closed_choice.py)
    const bool ring_pays = tune.ring == 1 || M == 4;
    if (!(want && ring_pays && NP >= 1 && nbuf >= 2 && ((long)M * gimg) % 4 == 0 && 16 * c.D * f.NTW <= kStageStride)) return false;
    ta.flat_img = gimg;
    ta.ring_np = NP; ta.ring_ns = NS; ta.ring_nc = NC; ta.ring_aw = AW; ta.ring_m = M; ta.ring_nbuf = (int)nbuf; ta.ring_parts = 1;
    ta.ring_ctr = f.ticket;
    ta.ring_tb = (int)((kRingTicketBytes + buf_bytes * 3 / 2 - 1) / (buf_bytes * 3 / 2));   // (a batch writes 1.5 x its buffer)
    if (ta.ring_tb < 2) ta.ring_tb = 2;
    if (tune.ring_tb > 0) ta.ring_tb = tune.ring_tb;
    while (2 * ta.ring_tb * M < NP) ++ta.ring_tb;
    r.family = TrajFamily::RingClosed;
    r.lds = fixed + (size_t)nbuf * buf_bytes + stage;
    r.blocks = at_most(((long)ta.G + M - 1) / M, f.num_cu);
    return true;
}

// episode-major producer / consumer pipeline (k_traj_pipe): where TrajFacts::pipe says so (plan_traj_shared)
static bool plan_pipe(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    if (!f.pipe) return false;
    const long units = (ta.G + kPipeGroups - 1) / kPipeGroups;
    r.family = TrajFamily::Pipe;
    r.lds = f.table_bytes;
    r.blocks = at_most(units, (long)f.num_cu * 6);                     // 5-wave workgroups: one resident round
    if (r.blocks >= 8) r.blocks = r.blocks / 8 * 8;                    // XCD-contiguous remap needs a multiple of 8
    ta.lean = units > 2 * (long)f.num_cu ? 1 : 0;                      // (see k_traj_pipe: 81 instead of 100 registers)
    r.gate = f.gated;
    r.lean = ta.lean && !f.gated;
    return true;
}

// serial-recurrence variants (DMP, closed loop): four (or two) groups per wave, recurrences in parallel on the lane
// quarters; needs its staging (52 / 26 KB) + the tables within 64 KB.  nq = groups per wave, 0 = declined (k_traj_stream).
// mpk_set_option "quad": 0 off, 2 force four, 3 force two, 4 force one (A/B runs, tests)
static bool plan_quarter(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const Tuning& tune = f.tune;
    const long num_cu = f.num_cu;
    // static staging (fp32 images) + the tables
    auto fits = [&](int nq) {
        return f.table_bytes + (4 * nq * kQuadImg) * sizeof(float) <= kLdsDefault;
    };
    const int quad_mode = tune.quad < 0 ? 1 : tune.quad;
    const long units4 = (ta.G + 3) / 4, units2 = (ta.G + 1) / 2;
    int nq = 0;
    // automatic (A/B-measured: profiles/r01_replan_end_to_end.md, profiles/r04_closed_loop.md):
    //   four per wave  while that gives two waves per SIMD AND the outputs still fit the memory-side cache (kWtBytes):
    //                  cfg3 DMP at B = 16384 33.8 us vs 38.7 with two; closed loop at 16384 30.8 vs 34.7, at 32768 56.7 vs
    //                  69.1 (round 4: 256 registers = two waves per SIMD; 271 = one before, and two groups won everywhere);
    //   two per wave   below that (one wave per SIMD exposes every LDS / MFMA latency: closed loop at B = 8192
    //                  20.4 -> 19.2 us) AND above it: at HBM-streaming sizes the launch is bound by its store pattern
    //                  (stores alone 153 of 166 us), and a four-group wave keeps 12 - 16 output streams open (DMP at
    //                  B = 32768 82.4 vs 78.5 us, at 262144 608 vs 595; closed loop at B = 65536 182 vs 166 us);
    //   one per wave   for the closed loop at a few thousand episodes (cfg4 episodes at B = 2048: 0.061 -> 0.052 ms)
    if (f.serial && quad_mode != 0) {
        if (quad_mode == 2) nq = fits(4) ? 4 : 0;
        else if (quad_mode == 3) nq = fits(2) ? 2 : 0;
        else if (quad_mode == 4) nq = fits(1) ? 1 : 0;
        else if (f.dmp && fits(4)) {
            // DMP (round 4, second session: sweep in steps of 2 048 episodes, profiles/r04_serial_quantization.md): the launches
            // are ROUNDS of resident waves -- two per SIMD with four groups per wave, three with two (cfg3's shape) -- and a
            // launch that needs one wave more than a round takes most of a second one: cfg3 at 18 432 episodes 53 us with four
            // groups (2 304 units for 2 048 places) against 42 with two.  Four groups per wave exactly where they fit ONE round and
            // two groups per wave would not (12 289 - 16 384 episodes of cfg3: 30.6 - 32.6 us against 38.5 - 38.9)
            if (units4 <= num_cu * 8 && units2 > num_cu * 12) nq = 4;
            else if (fits(2) && units2 >= num_cu * 6) nq = 2;      // (below: one group per wave, k_traj_stream -- cfg3 at 4 096: 17.0 vs 18.5 us)
        }
        // (closed loop, second session: ... and four per wave ALSO where two per wave would need a second round of resident waves
        // (two per SIMD) and four per wave fit one -- 8 193 - 16 383 episodes at 7 DoF: a launch with one wave too many for a
        // round takes most of another; 8 704: 26.7 -> 25.3 us, 12 288: 28.0 -> 26.6, 14 336: 33.5 -> 27.8)
        else if (fits(4) && f.out_bytes <= kWtBytes &&
                 (units4 >= num_cu * 8 || (f.closed && units2 > num_cu * 8 && units4 <= num_cu * 8))) nq = 4;
        else if (fits(2) && units2 >= num_cu * 4) nq = 2;
        else if (f.closed && fits(1)) nq = 1;
    }
    // validity gate: the lane-quarter closed-loop kernels (k_traj_quad / duo / mono: gate_pass) and k_traj_pipe run it, so a gated
    // launch that k_traj_pipe left takes one group per wave where the rule above took none
    // (a forced "quad" 0, or tables beyond the lane-quarter kernels' LDS: declined -- the caller's separate launches)
    if (f.gated && nq == 0 && f.serial && tune.quad != 0 && fits(1)) nq = 1;
    if (nq == 0) return false;
    r.family = TrajFamily::Quarter;
    r.nq = nq;
    r.gate = f.gated;
    r.lds = f.table_bytes + f.lds_pad;                                 // ("lds_pad": EXTRA dynamic LDS)
    const long units = (ta.G + nq - 1) / nq;
    r.blocks = (int)((at_most(units, f.max_waves) + 3L) / 4);
    if (r.blocks >= 8) r.blocks = (r.blocks + 7) / 8 * 8;
    // "serial_order" 1: short-lived workgroups in address order (one unit per wave); 2: persistent without the XCD remap
    if (tune.serial_order >= 1) {
        ta.inorder = 1;
        if (tune.serial_order == 1) r.blocks = (int)((units + 3) / 4);
    }
    return true;
}

// short-lived workgroups (k_traj_burst, "ring" 2): one batch of M groups per workgroup, WPG waves per group
static bool plan_burst(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const Tuning& tune = f.tune;
    if (!(f.episode_major && f.flat_ok && tune.ring == 2)) return false;
    int M = tune.ring_m > 0 ? tune.ring_m : 4;
    int WPG = tune.ring_np > 0 ? tune.ring_np : 1;
    if (M > 8) M = 8;
    if (M * WPG > 8) WPG = 8 / M < 1 ? 1 : 8 / M;
    const size_t bytes = (size_t)f.nst * M * f.flat_img * sizeof(float);
    if (f.table_bytes + bytes > kLdsPerCu) return false;
    ta.flat_img = f.flat_img;
    ta.burst = 1; ta.ring_m = M; ta.ring_np = WPG;
    r.family = TrajFamily::Burst;
    r.lds = f.table_bytes + bytes;
    r.blocks = (int)(((long)ta.G + M - 1) / M);
    return true;
}

// whole-trajectory images (k_traj_flat): open loop, promp / prodmp, aligned outputs, T * D a multiple of 4, and
// two workgroups' images + tables within a CU's LDS.  Automatic once the outputs stream to HBM (A/B on the
// streaming row, profiles/r03_streaming.md); mpk_set_option "flat": 0 off, 1 force
static bool plan_flat(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const DevCfg& c = f.c;
    const Tuning& tune = f.tune;
    if (!(f.episode_major && f.flat_ok && tune.flat != 0 && (tune.flat == 1 || (f.out_bytes > f.stream_from && tune.bulk < 0)))) return false;
    ta.flat_img = f.flat_img;
    // (write-through while the outputs fit the memory-side cache: kWtBytes)
    r.lds = f.lds_flat + f.lds_pad;                                      // "lds_pad": occupancy experiments
    // workgroups per CU: TWO, also where the LDS holds three (round 5: three -- twelve waves, twelve write streams per CU -- were
    // 7 - 20 % slower than two at every size from 12 288 to 1 M episodes of cfg2's trajectory-only shape: 32 768 episodes 33.5 ->
    // 31.2 us, 65 536: 73.0 -> 68.8, 262 144: 318 -> 260; with three arrays two were all that fitted, and one is slower again)
    // ("phase_waves" 4 / 8 / 12: one / two / three workgroups, for A/B runs)
    const long wg_cap = tune.phase_waves >= 4 ? tune.phase_waves / 4 : 2;
    const long wg = (long)(kLdsPerCu / r.lds) < wg_cap ? (long)(kLdsPerCu / r.lds) : wg_cap;
    const long resident = (long)f.num_cu * (wg < 1 ? 1 : wg) * 4;       // 4-wave workgroups, persistent
    // the DoF count compiled in for the shapes the reference registers MP environments with (k_traj_flat_d, mpk_traj_ring.h);
    // "ring_dbg" bit 64: the generic kernel (A/B runs, tests)
    const bool dof_compiled = (c.D == 5 || c.D == 7) && c.KP <= 8 && !(ta.ring_dbg & 64);
    if (dof_compiled) ta.burst = 2;
    r.family = dof_compiled ? TrajFamily::FlatD : TrajFamily::Flat;
    r.blocks = (int)((at_most(ta.G, resident) + 3L) / 4);
    if (r.blocks >= 8) r.blocks = (r.blocks + 7) / 8 * 8;                // XCD-contiguous remap needs a multiple of 8
    return true;
}

// episode-major, one group per wave (k_traj_stream), with or without bulk input staging
static bool plan_stream(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const DevCfg& c = f.c;
    const Tuning& tune = f.tune;
    if (!f.episode_major) return false;
    // bulk input staging: chunk blocks must be float4-sized / aligned and fit the per-lane register image
    const int EPC = kChunkGroups * f.NTW;
    const size_t img_floats = (size_t)EPC * (c.P + 2 * c.D + 4 * c.D);
    const size_t lds_bulk = f.table_bytes + 4 * 2 * img_floats * sizeof(float);
    const bool bulk_shape = (EPC * c.P) % 4 == 0 && (EPC * c.D) % 4 == 0 && (EPC * c.P) / 4 <= 128 && (EPC * c.D) / 2 <= 64 && f.in_ok &&
                            lds_bulk + 4 * kStageFloats * sizeof(float) <= kLdsDefault;
    // mpk_set_option "bulk": 0 disables, 2 forces it below the size threshold too (tests); default: HBM-streaming sizes only
    const int bulk_mode = tune.bulk < 0 ? 1 : tune.bulk;
    // automatic: only when the outputs stream to HBM AND the 4x coarser work units still fill the chip; the
    // latency-bound DMP recurrence prefers occupancy over input staging
    const long chunks = (ta.G + kChunkGroups - 1) / kChunkGroups;
    const bool auto_ok = f.out_bytes > kCachedBytes && chunks >= f.max_waves / 2 && !f.dmp;
    r.family = TrajFamily::Stream;
    r.bulk = bulk_shape && bulk_mode != 0 && (bulk_mode == 2 || auto_ok);
    r.lds = (r.bulk ? lds_bulk : f.table_bytes) + f.lds_pad;             // ("lds_pad": EXTRA dynamic LDS)
    long waves = at_most(r.bulk ? chunks : (long)ta.G, f.max_waves);
    if (tune.phase_waves > 0 && waves > (long)f.num_cu * tune.phase_waves) waves = (long)f.num_cu * tune.phase_waves;   // (A/B runs: waves per CU)
    r.blocks = (int)((waves + 3) / 4);
    if (r.blocks >= 8) r.blocks = (r.blocks + 7) / 8 * 8;                // XCD-contiguous remap needs a multiple of 8
    return true;
}

// tile-major (k_traj_tiles), and with the closed loop's serial role in front (k_traj_split): takes whatever is left
static void plan_tiles(const TrajFacts& f, TrajArgs& ta, TrajRoute& r) {
    const Tuning& tune = f.tune;
    const int NRT = f.NRT;
    const long items = (long)ta.G * NRT;
    long ipw = (items + f.max_waves - 1) / f.max_waves;                // items per wave, balanced
    if (tune.ipw > 0) ipw = tune.ipw;                                  // mpk_set_option "ipw" (A/B runs)
    // the kernel divides wave ids by NRT with a 32-bit multiply-high: exact while #waves < 2^32 / NRT
    const long wave_cap = (long)((1ull << 32) / (unsigned long long)NRT) - 8 * NRT;
    if ((items + ipw - 1) / ipw > wave_cap) ipw = (items + wave_cap - 1) / wave_cap;
    const long waves = (items + ipw - 1) / ipw;
    const int wpb = (tune.tiles_wpb == 1 || tune.tiles_wpb == 2) && !f.split ? tune.tiles_wpb : 4;   // A/B: smaller workgroups
    ta.wpb = wpb;
    int blocks = (int)((waves + wpb - 1) / wpb);
    {   // #waves % NRT == 0, and a multiple of 8 blocks for the XCD remap once there are that many
        int g8 = 8, rem = NRT;
        while (rem) { const int t = g8 % rem; g8 = rem; rem = t; }     // gcd(8, NRT)
        const int unit = blocks >= 8 ? NRT / g8 * 8 : NRT;             // lcm(8, NRT) or NRT
        blocks = (blocks + unit - 1) / unit * unit;
    }
    ta.gstride = blocks * wpb / NRT;
    ta.nrt_magic = NRT > 1 ? (unsigned)((1ull << 32) / (unsigned long long)NRT) + 1u : 0u;
    if (blocks < 1) blocks = 1;
    r.family = TrajFamily::Tiles;
    r.lds = f.lds_pad;                  // no dynamic LDS of their own ("lds_pad", A/B runs: caps the workgroups per CU)
    if (f.split) {
        // serial-role workgroups first (they are the long pole and must start first), capped at one resident round of the chip
        const int EPW = 64 >> ta.sh;                           // episodes per serial-role wave: one lane per (episode, DoF)
        const long units = ((long)f.B + EPW - 1) / EPW;
        ta.ser_blocks = (unsigned)at_most((units + 3) / 4, (long)f.num_cu * 8);
        blocks += (int)ta.ser_blocks;
        r.family = TrajFamily::Split;
    }
    r.blocks = blocks;
}

// what mpk_last_kernel reports: [kernel][MP type][none | fused actions | closed loop | closed loop + validity gate]
static const char* traj_kernel_name(const TrajRoute& r, int mp_type, bool act, bool closed) {
#define MPK_NAMES(k)                                                           \
    {{k "<promp>", k "<promp,act>", k "<promp,closed>", k "<promp,closed,gate>"}, \
     {k "<dmp>", k "<dmp>", k "<dmp>", k "<dmp>"},                                \
     {k "<prodmp>", k "<prodmp,act>", k "<prodmp,closed>", k "<prodmp,closed,gate>"}}
    static const char* const names[][3][4] = {
        MPK_NAMES("k_traj_tiles"), MPK_NAMES("k_traj_split"), MPK_NAMES("k_traj_stream"), MPK_NAMES("k_traj_flat"), MPK_NAMES("k_traj_burst"),
        MPK_NAMES("k_traj_quad"), MPK_NAMES("k_traj_duo"), MPK_NAMES("k_traj_mono"), MPK_NAMES("k_traj_pipe"), MPK_NAMES("k_traj_ring")};
#undef MPK_NAMES
    static_assert(MPK_MP_PROMP == 0 && MPK_MP_DMP == 1 && MPK_MP_PRODMP == 2, "the table's MP rows");
    int k = 0;
    switch (r.family) {
        case TrajFamily::Tiles: k = 0; break;
        case TrajFamily::Split: k = 1; break;
        case TrajFamily::Stream: k = 2; break;
        case TrajFamily::Flat: case TrajFamily::FlatD: k = 3; break;
        case TrajFamily::Burst: k = 4; break;
        case TrajFamily::Quarter: k = r.nq == 4 ? 5 : r.nq == 2 ? 6 : 7; break;
        case TrajFamily::Pipe: k = 8; break;
        case TrajFamily::RingOpen: case TrajFamily::RingClosed: k = 9; break;
    }
    return names[k][mp_type][r.gate ? 3 : closed ? 2 : act ? 1 : 0];
}

int plan_traj_shared(const DevCfg& c, const SharedTables& st, const TrajRequest& q, int num_cu, const Tuning& tune, unsigned* ticket,
                     int* fault, TrajArgs& ta, ActArgs& aa, TrajRoute& r) {
    const int B = q.B;
    TrajFacts f{c, tune};
    f.B = B; f.num_cu = num_cu; f.ticket = ticket;
    f.dmp = c.mp_type == MPK_MP_DMP;
    f.closed = q.q_state != nullptr;
    f.act = q.actions != nullptr;
    f.gated = q.gate != nullptr;     // validity gate: the lane-quarter closed-loop kernels (k_traj_quad / duo / mono: gate_pass) and k_traj_pipe
    const bool dmp = f.dmp, closed = f.closed, act = f.act, gated = f.gated;
    if (gated && !(closed && act)) { set_error("the validity gate belongs to the closed-loop step"); return MPK_EINVAL; }
    ta.fault = fault;
    ta.ring_dbg = tune.ring_dbg > 0 ? tune.ring_dbg : 0;
    // the bits that leave outputs unwritten (1 no production, 2 no stores, 128 a batch never published; open loop: 8 no input loads)
    // count only after mpk_set_option(.., "ablations", 1) -- measurements and fault injection, never by accident
    if (tune.ablations != 1) ta.ring_dbg &= ~(1 | 2 | 128 | (closed ? 0 : 8));
    fill_request_args(c, st, q, act, ta, aa);
    ta.pos = q.pos; ta.vel = q.vel; ta.actions = q.actions; ta.c_pos = q.c_pos; ta.c_vel = q.c_vel;
    const int NTW = f.NTW = 16 >> ta.sh;
    f.nst = 2 + (act ? 1 : 0);
    const int SEG = 16 * c.D, seg4 = SEG / 4, TD = f.TD = c.T * c.D;
    auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool ptr_ok = f.ptr_ok = aligned16(q.pos) && aligned16(q.vel) && (!act || aligned16(q.actions));
    f.in_ok = aligned16(q.params) && aligned16(q.init_pos) && aligned16(q.init_vel) && (!act || closed || (aligned16(q.c_pos) && aligned16(q.c_vel)));
    // T*D % 4 != 0: episodes start 0..3 floats past a 16-byte boundary -> shifted staging image (one spare chunk per
    // episode segment), if the segments of a group still fit the 64 lanes of a wave
    // (misaligned output pointers take the generic store path, whose staging image is never shifted)
    ta.shifted = (ptr_ok && TD % 4 != 0 && NTW * (seg4 + 1) <= 64 && NTW * (SEG + 4) <= kStageStride) ? 1 : 0;
    ta.td3 = TD & 3;
    ta.pitch = ta.shifted ? SEG + 4 : SEG;
    ta.cps = ta.shifted ? seg4 + 1 : seg4;
    ta.inv_cps = 65536u / (unsigned)ta.cps + 1u;
    ta.vec_ok = ptr_ok && (TD % 4 == 0 || ta.shifted);
    const int ct = act ? q.rc->controller_type + (closed ? 3 : 0) : -1;
    f.NRT = (c.T + 15) / 16;
    f.max_waves = (long)num_cu * 32;     // 8 waves per SIMD resident
    f.lds_pad = tune.lds_pad > 0 ? (size_t)tune.lds_pad * 1024 : 0;
    // work decomposition: episode-major once the outputs stop being cache resident (or when it is the only option)
    const size_t table_bytes = f.table_bytes = ((size_t)st.n_out * c.KP * st.TS + st.TS) * sizeof(float);
    const double out_bytes = f.out_bytes = (double)B * c.T * c.D * 4.0 * f.nst;
    const int ov = f.ov = tune.mapping == 1 || tune.mapping == 2 ? tune.mapping : 0;   // mpk_set_option "mapping"
    // closed loop, promp / prodmp, outputs cache resident: tile-major with a serial role (k_traj_split).  "split" 0 / 1
    // switches it off / forces it; a forced episode-major variant ("mapping" 2, "quad" 0 / 2 / 3 / 4, "bulk" 2) wins
    const bool variant_forced = ov == 2 || tune.quad == 0 || tune.quad >= 2 || tune.bulk == 2;
    // (its serial role stores actions as aligned float4 chunks: trajectories and the last row tile must be whole chunks)
    const int last_rows = c.T - (c.T - 1) / 16 * 16;
    const bool split_shape = ptr_ok && TD % 4 == 0 && (last_rows * c.D) % 4 == 0;
    // episode-major producer / consumer pipeline (k_traj_pipe): the default closed-loop kernel whenever its tables and
    // images fit; "pipe" 0 / 1 switches it off / forces it; "split" 1 forces the tile-major kernel with a serial role
    // Automatic up to three 5-wave workgroups per CU (B = 6144 at 7 DoF): measured against the best one-wave kernel
    // (profiles/r02_closed_loop.md) full step 10.1 vs 11.9 us at B = 2048, 11.8 vs 14.1 at 4096, 22.1 vs 19.7 at 8192;
    // 25-of-100-step plan 8.1 vs 8.8, 9.5 vs 11.6, 17.2 vs 16.5 -- beyond that the launch is store-bound and the barrier
    // per row tile only makes the store stream burstier.
    const bool pipe_fits = table_bytes + 2 * kPipeGroups * kQuadImg * sizeof(float) <= kLdsDefault;
    const long pipe_units = ((long)ta.G + kPipeGroups - 1) / kPipeGroups;
    // (with the validity gate -- k_traj_pipe<.., GATE>, 153 registers: two workgroups per CU -- only while ONE workgroup per CU holds the
    // launch: cfg5, us gated / ungated: 1 024 episodes 28.8 / 24.9 (k_traj_mono<.., gate>: 37.5), 2 048: 29.2 / 25.2, 4 096: 55.6 / 28.7)
    f.pipe = closed && !dmp && pipe_fits && tune.split != 1 &&
             (tune.pipe == 1 || (tune.pipe != 0 && !variant_forced && pipe_units <= (gated ? 1L : 3L) * num_cu));
    f.split = !f.pipe && closed && !gated && !dmp && split_shape && tune.split == 1;
    // (trajectory-only launches of the shapes k_traj_flat takes -- two workgroups of whole-trajectory images per CU -- go episode-major from
    // kFlatTrajBytes on: round 5, cfg2's shape, us tiles / flat: 8 192 episodes 10.7 / 11.0, 12 288: 14.5 / 14.1, 16 384: 19.2 / 18.2)
    f.flat_img = (NTW * TD + 3) / 4 * 4;
    f.lds_flat = table_bytes + (size_t)4 * f.nst * f.flat_img * sizeof(float);
    f.flat_ok = !closed && !dmp && ptr_ok && TD % 4 == 0 && f.lds_flat <= kLdsHalf;
    f.flat_takes_it = !act && f.flat_ok && tune.flat != 0;
    f.stream_from = f.flat_takes_it && tune.bulk < 0 ? kFlatTrajBytes : kCachedBytes;
    // the serial recurrences (DMP, closed loop) run episode-major whatever the size; a forced k_traj_split stays tile-major (its tiles
    // role needs that geometry).  Open loop, promp / prodmp: by the size of the outputs, "mapping" 1 / 2 forces tile- / episode-major,
    // a forced k_traj_flat / ring / burst ("flat" 1, "ring" 1 / 2) is episode-major where it applies
    f.serial = (dmp || closed) && !f.split;
    const bool open_episode_major = !dmp && !closed && (ov == 2 || tune.flat == 1 || tune.ring >= 1 || (ov != 1 && out_bytes > f.stream_from));
    const bool stream_fits = table_bytes + 4 * kStageFloats * sizeof(float) <= kLdsDefault;
    // the caller falls back: per-episode kernels for dmp, trajectory + rollout launches for the closed loop
    if (f.serial && !stream_fits) { set_error("trajectory too long for the episode-major kernel's LDS budget"); return MPK_ENOTIMPL; }
    f.episode_major = f.serial || (open_episode_major && stream_fits);

    // ---- the precedence: the first family that takes the launch has it ----
    r = TrajRoute{};
    r.ct = dmp ? -1 : ct;
    if (!(plan_ring_open(f, ta, r) || plan_ring_closed(f, ta, r) || plan_pipe(f, ta, r) || plan_quarter(f, ta, r))) {
        if (gated) return MPK_ENOTIMPL;       // the gate runs in k_traj_pipe and the lane-quarter kernels only
        if (!(plan_burst(f, ta, r) || plan_flat(f, ta, r) || plan_stream(f, ta, r))) plan_tiles(f, ta, r);
    }
    if (r.blocks < 1) r.blocks = 1;
    const bool tile_major = r.family == TrajFamily::Tiles || r.family == TrajFamily::Split;
    if (tile_major && ta.gstride <= 0) { set_error("internal: tile-major launch without its group stride"); return MPK_EINVAL; }
    // write-through stores for the cache-resident tile-major case, and for the episode-major kernels while the outputs fit the
    // memory-side cache (kWtBytes); mpk_set_option "write_through" overrides, for A/B runs
    bool wt = tune.write_through >= 0 ? tune.write_through != 0 : (tile_major || out_bytes <= kWtBytes);
    // write-through stores address an output array through one buffer resource with 32-bit byte offsets (wt_store16): arrays
    // of 2 GiB and more (never cache resident anyway; only a forced option gets here) take plain stores
    if ((double)B * c.T * c.D * 4.0 >= 2147483648.0) wt = false;
    r.write_through = tile_major && wt;
    ta.wt = !tile_major && wt ? 1 : 0;
    // (a gated DMP handle: the lane-quarter kernel is named as promp rows, then declined -- the caller's separate launches take it)
    r.name = traj_kernel_name(r, gated && dmp ? MPK_MP_PROMP : c.mp_type, act, closed);
    return gated && dmp ? MPK_ENOTIMPL : MPK_OK;
}

int launch_traj_shared(const DevCfg& c, const SharedTables& st, const TrajRequest& q, const LaunchSite& at) {
    TrajArgs ta{};
    ActArgs aa{};
    TrajRoute r{};
    const int rc_ = plan_traj_shared(c, st, q, at.num_cu, at.tune, at.ticket, at.fault, ta, aa, r);
    if (r.name) *at.kernel_name = r.name;
    if (rc_ != MPK_OK) return rc_;
    switch (r.family) {
        case TrajFamily::RingOpen: case TrajFamily::RingClosed: case TrajFamily::Burst: case TrajFamily::FlatD:
            return by_mp_type(c.mp_type, [&](auto mp) { return launch_traj_ring<decltype(mp)::value>(ta, aa, r, at.stream); });
        default:
            return by_mp_type(c.mp_type, [&](auto mp) { return launch_traj_ct<decltype(mp)::value>(ta, aa, r, at.stream); });
    }
}
#endif  // MPK_DEVICE_ONLY

}  // namespace mpk
