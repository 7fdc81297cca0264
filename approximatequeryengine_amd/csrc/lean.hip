// lean.hip — k_sweep_lean / k_sweep_lean_multi: every round of a multi-round (CLT) query in ONE lean launch, judged once
// at the end — and a batch of such queries in one launch, a group of workgroups each.
//
// The reference's monitor (custom_bplus_db.cpp:885-1043) re-evaluates its rules while the pointer threads are still
// walking, so that they can stop early (DB.cpp:930, 987).  k_sweep_persist (persist.hip) keeps that shape: a monitor
// wave judges rounds as they complete and raises should_stop.  On a table of 10 M rows there is nothing left to stop:
// every wave holds its tile in flight from the first microsecond, the sweep is over after five, and what the query then
// waits for is the hand-off.  This kernel is for those queries — and for longer sweeps that are predicted not to stop
// early (plans.hip, launch_form) — provided every family of the plan is a plain run of rows, which is what strided
// pointers read through their stride-major views are.  It is built for a short critical path:
//
//   * no monitor wave, no polling, no stop word: every wave sweeps.  Workgroup b owns the tiles [b K, (b + 1) K) of the
//     launch's list (K = tiles / workgroups, rounded up; its wave j takes the j-th, (j + 16)-th, ... of them: the 16 waves
//     stream one window of the column), so it sweeps tiles of one round, or of a few consecutive ones; it publishes ONE
//     56-byte partial per round it swept tiles of (sc1 stores, drained) and draws ONE ticket (sharded counters, as k_round);
//   * the workgroup that draws the last ticket sums every round's slots of the flat partial list — fewer than
//     workgroups + rounds of them, whatever the size of the sweep — in a fixed order (bit-reproducible), 64 threads per
//     round, and wave 0 then judges EVERY round at once, lane q evaluating the rules on the moments through round q
//     (DB.cpp:936-961, 993-1016).  The first round that satisfies a rule — or the last — is the query's answer: a
//     decision is a pure function of the partials, so the rounds swept beyond it change nothing;
//   * the tile decode is a dozen instructions: lane i of every wave holds runs i and i + 64 of the plan in registers (one batch of
//     loads in the prologue), the run of a tile is found by one wave-wide comparison and read with v_readlane; tiles
//     that lie inside their run — all but a run's last — take no masks.  With four waves per SIMD every instruction of
//     a wave costs ~8 ns of wall time while all waves do the same thing, which they do at the start and at the end of a
//     short query: k_sweep_persist's general tile path (~500 vector instructions of window arithmetic per tile) had the
//     first tile of a 10 M-row query folded after 3.3 us and the last after 8.3, where a lean loop needs 0.4 and 3.7
//     (tools/exp_latency.hip) — 17.7 us per launch against 9.5.
//
// Plans of more runs than the lanes hold (up to 512: 64 ... 256 pointers on 10 M rows) take the WIDE instantiation: the
// table goes through LDS, one copy per workgroup, and a tile's run is found by bisection.
//
// Same forms as the persistent sweep (PersistLaunch): decisions in the kernel, the head form (rounds + the top-up as
// one more slot, `more_rounds`), totals only (multi-GPU: every slot's total for the all-reduce).  Nothing in it waits
// for another workgroup, so the groups of a batch (k_sweep_lean_multi) may outnumber the compute units.
#include <hip/hip_ext.h>

#include "device_common.hpp"

namespace aqe {
namespace {

#define AQE_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

typedef const AQE_KARG LeanLaunch* LeanKarg;

// Diagnostics (builds with -DAQE_LEAN_STAMPS only; tools/stamp_lean.py, tools/stamp_union.py): s_memrealtime marks, 100 MHz.
// [wave][8] of the first kMaxPersistGrid workgroups: 0 entry, 1 table in registers, 2 first tile folded, 3 sweep done, 4 sums
// handed to the workgroup, 5 partial out (wave 0), 6 ticket drawn (wave 0);  then [8] of the folding workgroup: 1 rounds
// summed, 2 judged.  A union group (lean_union) marks 0 entry, 1 tile list in registers, 2 first tile folded, 3 sweep done,
// 5 partials out, 6 ticket drawn; its fold 3 partial list staged, 4 pieces summed, 5 targets summed, and then per judging
// wave [wave][8]: 0 first judge done, 1 last result sent, 2 the wave's hardware id (HW_ID: bits 5:4 its SIMD).
#ifdef AQE_LEAN_STAMPS
// (-DAQE_LEAN_STAMPS=2, tools/stamp_overlap.py: two blocks of marks, a launch writes block `epoch & 1` — consecutive launches of a
// context keep their marks apart, on one clock)
#if AQE_LEAN_STAMPS + 0 >= 2
#define LEAN_STAMP_BLOCKS 2
#define LEAN_STAMP_BASE (static_cast<size_t>(epoch & 1ull) * kLeanStampWords)
#else
#define LEAN_STAMP_BLOCKS 1
#define LEAN_STAMP_BASE static_cast<size_t>(0)
#endif
constexpr size_t kLeanStampWords = (static_cast<size_t>(kMaxPersistGrid) * kPersistWaves + 1 + kPersistWaves) * 8;
__device__ unsigned long long g_lean_stamps[LEAN_STAMP_BLOCKS * kLeanStampWords];
#define LEAN_STAMP(slot) do { if (lane == 0 && blockIdx.x < static_cast<unsigned>(kMaxPersistGrid)) g_lean_stamps[LEAN_STAMP_BASE + (static_cast<size_t>(blockIdx.x) * kPersistWaves + wave) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define LEAN_STAMP_FOLD(slot) do { if (threadIdx.x == 0) g_lean_stamps[LEAN_STAMP_BASE + static_cast<size_t>(kMaxPersistGrid) * kPersistWaves * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define LEAN_STAMP_JUDGE(slot) do { if (lane == 0) g_lean_stamps[LEAN_STAMP_BASE + (static_cast<size_t>(kMaxPersistGrid) * kPersistWaves + 1 + wave) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
// (s_getreg_b32 hwreg(HW_REG_HW_ID, 0, 32): a read of the wave's placement)
#define LEAN_STAMP_HWID(slot) do { if (lane == 0) g_lean_stamps[LEAN_STAMP_BASE + (static_cast<size_t>(kMaxPersistGrid) * kPersistWaves + 1 + wave) * 8 + (slot)] = __builtin_amdgcn_s_getreg((31 << 11) | 4); } while (0)
#else
#define LEAN_STAMP(slot) do { } while (0)
#define LEAN_STAMP_FOLD(slot) do { } while (0)
#define LEAN_STAMP_JUDGE(slot) do { } while (0)
#endif

__device__ __forceinline__ void lean_state_store(QueryState* g, const QueryState& st) {
    static_assert(sizeof(QueryState) % 8 == 0, "state is moved as 8-byte words");
    const unsigned long long* s = reinterpret_cast<const unsigned long long*>(&st);
    unsigned long long* d = reinterpret_cast<unsigned long long*>(g);
#pragma unroll
    for (unsigned i = 0; i < sizeof(QueryState) / 8; ++i) __hip_atomic_store(d + i, s[i], AQE_RLX);
}

__device__ __forceinline__ u64 read_lane_u64(u64 v, unsigned src_lane) {
    const unsigned lo = __builtin_amdgcn_readlane(static_cast<unsigned>(v), src_lane);
    const unsigned hi = __builtin_amdgcn_readlane(static_cast<unsigned>(v >> 32), src_lane);
    return (static_cast<u64>(hi) << 32) | lo;
}

__device__ __forceinline__ u64* lean_t0_word(unsigned* counter) { return reinterpret_cast<u64*>(counter + kShards * kShardStride + 8); }

struct __attribute__((packed, aligned(8))) Row2 { double x, y; };

// One tile = up to 1024 consecutive rows from `base` (two rows per lane per 16-byte load, eight loads in flight);
// `rem` rows of the run (or of the block) are left from `base` on.
template <bool kNT>
__device__ __forceinline__ void lean_tile(const double* base, unsigned rem, const double* safe, int lane, int has_where, double wmin, double wmax,
                                          double shift, TileAcc& ta) {
    Row2 v2[kTileUnroll];
    if (rem >= static_cast<unsigned>(kDenseTileOrdinals)) {  // inside the run: no masks
        const Row2* const p = reinterpret_cast<const Row2*>(base) + lane;
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            if (kNT) {  // a sweep beyond the Infinity Cache: past the caches (device_common.hpp, sweep_family)
                v2[k].x = __builtin_nontemporal_load(&p[k * 64].x);
                v2[k].y = __builtin_nontemporal_load(&p[k * 64].y);
            } else {
                v2[k] = p[k * 64];
            }
        }
        ta.nv = 2u * kTileUnroll;
        if (has_where) {
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const double x = v2[k].x, y = v2[k].y;
                const bool px = x >= wmin && x <= wmax, py = y >= wmin && y <= wmax;  // inclusive both ends, DB.cpp:329
                const double dx = px ? x - shift : 0.0, dy = py ? y - shift : 0.0;
                ta.n += (px ? 1u : 0u) + (py ? 1u : 0u);
                ta.s += dx; ta.q += dx * dx;
                ta.s += dy; ta.q += dy * dy;
            }
        } else {
            ta.n = 2u * kTileUnroll;
#pragma unroll
            for (int k = 0; k < kTileUnroll; ++k) {
                const double dx = v2[k].x - shift, dy = v2[k].y - shift;
                ta.s += dx; ta.q += dx * dx;
                ta.s += dy; ta.q += dy * dy;
            }
        }
        return;
    }
    // the last tile of a run — every tile of a run of 1000-row blocks: the same 16-byte loads, a pair masked where it
    // leaves the run and never addressed there (such a lane reads rows 0 and 1 of the column instead)
    bool ok[kTileUnroll];
#pragma unroll
    for (int k = 0; k < kTileUnroll; ++k) {
        const unsigned oi = 2u * static_cast<unsigned>(lane) + 128u * static_cast<unsigned>(k);
        ok[k] = oi + 1u < rem;  // both rows of the pair inside the run
        const Row2* const p = reinterpret_cast<const Row2*>(ok[k] ? base + oi : safe);
        if (kNT) {
            v2[k].x = __builtin_nontemporal_load(&p->x);
            v2[k].y = __builtin_nontemporal_load(&p->y);
        } else {
            v2[k] = *p;
        }
    }
#pragma unroll
    for (int k = 0; k < kTileUnroll; ++k) {
        const double x = v2[k].x, y = v2[k].y;
        const bool px = ok[k] && (!has_where || (x >= wmin && x <= wmax)), py = ok[k] && (!has_where || (y >= wmin && y <= wmax));
        const double dx = px ? x - shift : 0.0, dy = py ? y - shift : 0.0;
        ta.nv += ok[k] ? 2u : 0u;
        ta.n += (px ? 1u : 0u) + (py ? 1u : 0u);
        ta.s += dx; ta.q += dx * dx;
        ta.s += dy; ta.q += dy * dy;
    }
    if (rem & 1u) {  // (wave-uniform) a run of odd length ends in half a pair: that row on its own, folded by lane 0
        const double x = base[rem - 1u];
        const bool px = lane == 0 && (!has_where || (x >= wmin && x <= wmax));
        const double dx = px ? x - shift : 0.0;
        ta.nv += lane == 0 ? 1u : 0u;
        ta.n += px ? 1u : 0u;
        ta.s += dx; ta.q += dx * dx;
    }
}

// A tail's words, and a result's with its check word after them, as they lie in a judging wave's LDS
constexpr unsigned kLeanTailWords = sizeof(LeanTail) / 8u, kLeanResWords = sizeof(aqe_result) / 8u + 1u;

// Wave 0 of the folding workgroup, lane q holding the moments through round q (or a slot's own total where the form
// asks for that): the decision and the result.  The rules and what follows them are the monitor's (persist.hip,
// monitor_fold), evaluated once, for every round at the same time.  T: the launch's tail, in LDS.  kLanes = 32, 16, 8:
// each aligned row of kLanes lanes judges a member of its own (lean_union), lane q of the row holding round q, T the
// row's tail, res_words the row's words — such members have no top-up slot (plans.hip, union_groups).
template <unsigned kLanes = 64>
__device__ __forceinline__ void lean_judge(const LeanTail& T, const double (&tot)[7], const unsigned wave_lane, unsigned long long t0, unsigned long long epoch, unsigned long long* res_words) {
    static_assert(kLanes == 64 || kLanes == 32 || kLanes == 16 || kLanes == 8, "a whole wave per member, or an aligned row of its lanes");
    const unsigned lane = wave_lane & (kLanes - 1u), base = wave_lane & ~(kLanes - 1u) & 63u;  // lane in the member's lanes; their first
    const unsigned rounds = T.rounds;
    const bool tslot = kLanes == 64 && T.topup_slot != 0;  // the last slot is the top-up: summed on its own, never judged
    const unsigned rounds_j = rounds - (tslot ? 1u : 0u);
    if (T.totals_only) {  // multi-GPU form: hand the slot totals out; the decision is taken after the all-reduce
        if (lane < rounds) {
            double* o = T.out_totals + static_cast<size_t>(lane) * kVec;
#pragma unroll
            for (int cc = 0; cc < 7; ++cc) o[cc] = tot[cc];
            o[7] = 0.0;
        }
        return;
    }
    const FoldParams fp = T.fold;
    const FinalizeParams fin = T.fin;
    const bool with_result = T.finalize_here != 0;
    QueryState st{};
    st.n_a = tot[0]; st.sd_a = tot[1]; st.qd_a = tot[2];
    st.n_b = tot[3]; st.sd_b = tot[4]; st.qd_b = tot[5];
    st.n_p = tot[0] + tot[3]; st.sd_p = tot[1] + tot[4]; st.qd_p = tot[2] + tot[5];
    st.visited = tot[6];
    double tup[7] = {0, 0, 0, 0, 0, 0, 0};  // the top-up slot's own total
    if (tslot) {
#pragma unroll
        for (int cc = 0; cc < 7; ++cc) tup[cc] = read_lane_f64(tot[cc], static_cast<int>(rounds - 1u));
    }
    int code = 0;
    aqe_result res{};
    // every lane works its round's estimate out beside the rules: the two chains of f64 operations overlap (with a
    // top-up slot the estimate depends on the decision and follows it)
    const bool result_now = with_result && !tslot;
#ifndef AQE_ABL_NOJUDGE
    if (lane < rounds_j) {
        if (fp.is_clt) code = clt_rules(tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], fp);
        if (result_now) res = make_result(st, fin);
    }
#else
    res.sum = st.sd_p; res.n = static_cast<uint64_t>(st.n_p);
#endif
    const unsigned long long stops = kLanes == 64 ? __ballot(code != 0) : (__ballot(code != 0) >> base) & ((1ull << (kLanes & 63u)) - 1ull);
    const unsigned last_round = stops ? static_cast<unsigned>(__builtin_ctzll(stops)) : rounds_j - 1u;  // the rule holds after this round / samples exhausted
    if (lane != last_round) return;
    st.rounds = static_cast<int32_t>(last_round + 1u);
    st.converged = code;
    st.stop = code != 0;
    // DB.cpp:1032: too few rows collected -> the top-up is due.  Swept with the rounds (head form): it is added here.
    // Otherwise the result is marked and the host launches it (rarely due).
    const bool goes_on = code == 0 && T.more_rounds;  // head form: out of rounds, not out of samples
    bool due = T.topup_gate && st.n_p < static_cast<double>(fp.base / 4);
    if (tslot && due && !goes_on) {  // the fold of a top-up vector (device_common.hpp, fold)
        st.n_p += tup[0]; st.sd_p += tup[1]; st.qd_p += tup[2];
        st.topup += tup[0];
        st.visited += tup[6];
        due = false;
    }
    if (with_result && !result_now) res = make_result(st, fin);
    if (T.want_ticks) {
        st.t0 = t0;
        res.kernel_ms = static_cast<double>(__builtin_amdgcn_s_memrealtime() - st.t0) * 1e-5;
    }
    res.rounds = st.rounds;
    res.converged = code;
    res.topup_pending = goes_on ? 2 : due ? 1 : 0;  // 2: the host launches the plan's remaining rounds
#ifdef AQE_ABL_NOSTORE  // (ablation: everything computed, ONE 8-byte store to device memory)
    T.state->n_a = res.value + res.ci_lower + st.n_p + static_cast<double>(result_check(res, epoch) & 0xffu);
    return;
#endif
#ifdef AQE_ABL_RESDEV  // (ablation: the result into device memory instead of the pinned host block)
    lean_state_store(T.state, st);
    *reinterpret_cast<aqe_result*>(reinterpret_cast<char*>(T.state) + 256) = res;
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(T.state) + 512), result_check(res, epoch), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
#endif
    // The state is read by a later LAUNCH of the same execution only — the top-up when it is due (launched by fetch(), or
    // already enqueued behind this launch: keep_state), the remaining rounds of a head form — and by the stepwise forms,
    // which do not come here: otherwise its fourteen stores stay home (a store instruction costs one lane what it costs
    // sixty-four: ~25 ns each on this path).
    if (due || goes_on || T.keep_state || !with_result) lean_state_store(T.state, st);
    if (with_result) {
        // The result leaves as ONE store instruction: the finishing lane parks its words in LDS (cheap), lane i of the wave
        // sends word i.  The host polls the pinned result instead of waiting for the end of the launch: the check word
        // tells it when every field has landed (kernels.hpp, result_check).
        static_assert(sizeof(aqe_result) % 8 == 0 && sizeof(aqe_result) / 8 < 63, "one word per lane, the check word after them");
        *reinterpret_cast<aqe_result*>(res_words) = res;
        res_words[sizeof(aqe_result) / 8] = result_check(res, epoch);
    }
#ifdef AQE_LEAN_STAMPS
    g_lean_stamps[LEAN_STAMP_BASE + static_cast<size_t>(kMaxPersistGrid) * kPersistWaves * 8 + 2] = __builtin_amdgcn_s_memrealtime();
#endif
}

// (all lanes of wave 0, after lean_judge: lane i sends word i of the result, lane sizeof/8 the check word; kLanes = 32:
// lane i of each half, for its member; kLanes = 16, 8: T and res_words are the wave's FIRST row's, the other rows' follow
// them kLeanTailWords / kLeanResWords apart, and the wave sends the words of all its 64 / kLanes rows, 64 per store
// instruction, a result's check word after its words)
template <unsigned kLanes = 64>
__device__ __forceinline__ void lean_send_result(const LeanTail& T, const unsigned long long* res_words, const unsigned wave_lane) {
    const unsigned lane = wave_lane & (kLanes - 1u);
#if defined(AQE_ABL_NOSTORE) || defined(AQE_ABL_RESDEV)
    return;
#endif
    if constexpr (kLanes <= 16) {
        constexpr unsigned kRows = 64u / kLanes, kAll = kRows * kLeanResWords;
#pragma unroll
        for (unsigned x0 = 0; x0 < kAll; x0 += 64u) {
            const unsigned x = x0 + wave_lane, row = x / kLeanResWords, word = x - row * kLeanResWords;
            if (x >= kAll) continue;
            const LeanTail& Tr = *reinterpret_cast<const LeanTail*>(reinterpret_cast<const u64*>(&T) + row * kLeanTailWords);
            if (Tr.totals_only || !Tr.finalize_here) continue;  // (a row past the last member: a tail of zeros)
            unsigned long long* const to = word + 1u < kLeanResWords ? reinterpret_cast<unsigned long long*>(Tr.result) + word : Tr.result_seq;
            __hip_atomic_store(to, res_words[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    if (T.totals_only || !T.finalize_here) return;
    constexpr unsigned kWords = sizeof(aqe_result) / 8;
    if (lane < kWords) __hip_atomic_store(reinterpret_cast<unsigned long long*>(T.result) + lane, res_words[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if (lane == kWords) __hip_atomic_store(T.result_seq, res_words[kWords], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One lane of a workgroup that has published its partials: its ticket.  1 for the last of the G workgroups to arrive.
// At most 256 arrivals: 16 shards of 16 (a same-address atomic serialises at ~16 ns), then the top counter.
__device__ __forceinline__ int lean_ticket(unsigned* const counter, const unsigned bid, const unsigned G) {
    int last = 0;
    unsigned* const ct = counter + static_cast<size_t>(kShards) * kShardStride;
    constexpr unsigned kLeanShards = 16;
    if (G <= kLeanShards) {
        if (__hip_atomic_fetch_add(ct, 1u, AQE_RLX) == G - 1u) { __hip_atomic_store(ct, 0u, AQE_RLX); last = 1; }
    } else {
        const unsigned sh = bid % kLeanShards;
        const unsigned members = (G - sh + kLeanShards - 1u) / kLeanShards;
        unsigned* const cs = counter + static_cast<size_t>(sh) * kShardStride;
        if (__hip_atomic_fetch_add(cs, 1u, AQE_RLX) == members - 1u) {
            __hip_atomic_store(cs, 0u, AQE_RLX);
            if (__hip_atomic_fetch_add(ct, 1u, AQE_RLX) == kLeanShards - 1u) { __hip_atomic_store(ct, 0u, AQE_RLX); last = 1; }
        }
    }
    return last;
}

// The judges of a union group's fold (lean_union), kW lanes per member — the smallest of 8, 16 and 32 that holds the rounds
// of every member of the union: an aligned row of kW lanes judges one member, lane q of it holding the moments through
// round q, so a wave judges 64 / kW members at once.  Sixteen waves running lean_judge's chain of f64 operations side
// by side, four to a SIMD, take as long as their SIMD needs for four of them, however few lanes are live: with rows of
// 8 or 16 lanes only waves 0 .. kUnionDenseWaves - 1 judge — consecutive waves of a workgroup sit on different SIMDs —
// and with rows of 32 (a member may have kMaxPersistRounds = 32 rounds) all of them do.  Pass k: wave w judges members
// (waves k + w) 64 / kW and on — the bench's 32 members of 5 rounds in ONE pass of four waves.  `tails`, `results`: a
// slot per member of a pass (member m: slot m mod kUnionJudgeSlots — always one of its wave's own), the first
// kUnionJudgeSlots members' tails staged by the fold; a later pass fetches its tails first.  `rows`: the classes' rows of
// round totals.  The scan over rounds adds in ONE association whatever the width: row_shr by 1, 2, 4 (and 8, and the carry
// of the first sixteen into the second), a lane that would pull from below its row adding 0.0.
template <unsigned kW>
__device__ __forceinline__ void lean_union_judge(const LeanLaunch* const members, const unsigned nmem, const unsigned wave, const int lane,
                                                 const double* const rows, u64* const tails, unsigned long long* const results,
                                                 const unsigned long long epoch) {
    constexpr unsigned kPer = 64u / kW, kWaves = kW == 32 ? static_cast<unsigned>(kPersistWaves) : static_cast<unsigned>(kUnionDenseWaves);
    constexpr unsigned kPassWords = kPer * kLeanTailWords, kFetch = (kPassWords + 63u) / 64u;
    static_assert(kUnionJudgeSlots % (kWaves * kPer) == 0, "a wave's members of every pass fall into its own slots");
    if (wave >= kWaves) return;
    const unsigned row = static_cast<unsigned>(lane) / kW, q = static_cast<unsigned>(lane) % kW;
    for (unsigned m0 = wave * kPer; m0 < nmem; m0 += kWaves * kPer) {
        const unsigned slot0 = m0 % kUnionJudgeSlots;
        u64* const my_tails = tails + slot0 * kLeanTailWords;
        if (m0 >= static_cast<unsigned>(kUnionJudgeSlots)) {  // (uniform) a later pass: its tails, one round trip
            u64 w[kFetch];
#pragma unroll
            for (unsigned j = 0; j < kFetch; ++j) {
                const unsigned x = static_cast<unsigned>(lane) + 64u * j, m = m0 + x / kLeanTailWords;
                w[j] = x < kPassWords && m < nmem ? reinterpret_cast<const u64*>(&members[m].tail)[x % kLeanTailWords] : 0ull;
            }
            wave_lds_handoff();
#pragma unroll
            for (unsigned j = 0; j < kFetch; ++j) {
                const unsigned x = static_cast<unsigned>(lane) + 64u * j;
                if (x < kPassWords) my_tails[x] = w[j];
            }
            wave_lds_handoff();
        }
        // (a row past the last member reads a tail of zeros: no rounds, nothing judged, nothing sent)
        const LeanTail& Tm = *reinterpret_cast<const LeanTail*>(my_tails + row * kLeanTailWords);
        unsigned long long* const lds_res = results + (slot0 + row) * kLeanResWords;
        const unsigned rounds = Tm.rounds;
        const bool mine = q < rounds;
        const double* const r = rows + static_cast<size_t>(Tm.union_row + (mine ? q : 0u)) * 8u;
        double tot[7];
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) tot[cc] = mine ? r[cc] : 0.0;
        tot[6] = mine ? r[6] + r[7] : 0.0;
#pragma unroll
        for (int cc = 0; cc < 7; ++cc) {  // lane q of a row: the moments through round q (lean_query's scan, one row per round)
            // (a row of sixteen lanes shifts zeros in by itself; a row of eight that is the upper half of one does not)
            auto below = [&](double v, unsigned by) { return kW >= 16 || q >= by ? v : 0.0; };
            double p = tot[cc];
            p += below(dpp_f64<0x111>(p), 1u);
            p += below(dpp_f64<0x112>(p), 2u);
            p += below(dpp_f64<0x114>(p), 4u);
            if constexpr (kW >= 16) p += dpp_f64<0x118>(p);
            if constexpr (kW == 32) {
                const double carry = __shfl(p, static_cast<int>((static_cast<unsigned>(lane) & 32u) | 15u), 64);  // the half's first row's total
                p += (lane & 16) ? carry : 0.0;
            }
            tot[cc] = p;
        }
        lean_judge<kW>(Tm, tot, static_cast<unsigned>(lane), 0ull, epoch, lds_res);
        wave_lds_handoff();
#ifdef AQE_LEAN_STAMPS
        if (m0 == wave * kPer) { LEAN_STAMP_JUDGE(0); LEAN_STAMP_HWID(2); }
#endif
        // (rows of 8 or 16: the wave's rows are sent together, from its first row's tail and words on)
        if constexpr (kW == 32) lean_send_result<32>(Tm, lds_res, static_cast<unsigned>(lane));
        else lean_send_result<kW>(*reinterpret_cast<const LeanTail*>(my_tails), results + slot0 * kLeanResWords, static_cast<unsigned>(lane));
        LEAN_STAMP_JUDGE(1);
    }
}

// A UNION GROUP of a batch (plans.hip, build_union): sweep classes that read the same view with the same shift and WHERE
// bounds, swept as one.  The union of their runs is cut into PIECES — slot ranges over which one multiset of (class,
// round, pointer group) targets covers every slot — and tiled in 1024-slot tiles over the covered spans (from an even
// slot: every 16-byte load aligned; the gaps between spans are skipped).  Workgroup b sweeps the contiguous share
// [b K, (b + 1) K) of the tiles, as a multi-round query does, with ONE accumulator per piece (n, S, Q, rows: a piece feeds
// the same moments to every target that covers it), flushed when the piece changes as a round's is when the round
// changes.  A tile inside one piece takes lean_tile's unmasked path; a tile that crosses a piece boundary or a span's end
// is loaded once and summed per piece under row masks (a pair may be split).  The workgroup publishes one partial per piece
// it holds slots of and draws one ticket; the last one folds: the partials per piece in workgroup order, the pieces into
// the targets in ascending piece order, the targets into each class's rows of round totals — and from there every member
// is judged as lean_query judges a class's.  Fixed orders throughout: bit-reproducible.
template <bool kNT>
__device__ __forceinline__ void lean_union(const LeanLaunch& a, const LeanUnion* const U, const LeanLaunch* const members, const unsigned nmem,
                                           const unsigned bid, const unsigned G, const unsigned long long epoch,
                                           double (&lds_part)[kMaxPersistRounds][kPersistWaves][kVec], double (&lds_round)[kMaxPersistRounds][kVec],
                                           unsigned (&lds_mask)[kPersistWaves], int& s_last) {
    static_assert(kUnionWgPieces <= kMaxPersistRounds && kUnionWgPieces <= 32, "a share's pieces: a row of lds_part and a mask bit each");
    static_assert(sizeof(LeanUnion) + sizeof(unsigned) <= sizeof(lds_round), "the union's header is staged in lds_round, the largest round count after it");
    unsigned* const lds_max_rounds = reinterpret_cast<unsigned*>(&lds_round[0][0]) + sizeof(LeanUnion) / sizeof(unsigned);  // (the fold's)
    const int lane = threadIdx.x & 63;
    const unsigned wave = threadIdx.x >> 6;
    const unsigned t_lo = bid * a.tiles_per_wg;
    const unsigned t_end = t_lo + a.tiles_per_wg < a.ntiles ? t_lo + a.tiles_per_wg : a.ntiles;
    // the share's tiles: lane j of wave w holds tile t_lo + w + 16 j (one batch of loads, as the run table in lean_query)
    const u64* const tile_row = reinterpret_cast<const u64*>(U + 1);
    const unsigned* const tile_meta = reinterpret_cast<const unsigned*>(tile_row + a.ntiles);
    const unsigned* const wg = tile_meta + ((a.ntiles + 1u) & ~1u) + static_cast<size_t>(bid) * (kUnionWgPieces + 1);
    const unsigned my_t = t_lo + wave + kPersistWaves * static_cast<unsigned>(lane);
    u64 my_row = 0;
    unsigned my_meta = 0;
    if (my_t < t_end) { my_row = tile_row[my_t]; my_meta = tile_meta[my_t]; }
    const unsigned p0 = __builtin_amdgcn_readfirstlane(wg[0]);  // the share's first piece: its pieces are p0, p0 + 1, ...
    unsigned my_entry = 0;  // (wave 0) lane j: where the share's partial of piece p0 + j goes
    if (wave == 0 && lane < kUnionWgPieces) my_entry = wg[1 + lane];
#ifdef AQE_LEAN_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    LEAN_STAMP(1);
#endif
    // what only the folding workgroup reads, fetched now (lean_query): the union's header (the members' tails come with the
    // fold's one batch of loads)
    const bool head_stager = wave == kPersistWaves - 2u;
    u64 head_word = 0;
    if (head_stager && static_cast<unsigned>(lane) < sizeof(LeanUnion) / 8u) head_word = reinterpret_cast<const u64*>(U)[lane];
#pragma unroll
    for (unsigned i = 0; i < kMaxPersistRounds * kVec / 64; ++i) {
        const unsigned x = static_cast<unsigned>(lane) + 64u * i;
        lds_part[x >> 3][wave][x & 7u] = 0.0;
    }

    double ps = 0.0, pq = 0.0;
    unsigned pn = 0, pv = 0, cur = ~0u, touched = 0;  // the piece this wave is in; the share's pieces it has been in
    auto take = [&](unsigned piece, const TileAcc& ta) {
        if (piece != cur) {
            if (cur != ~0u) {
                const double v[7] = {static_cast<double>(pn), ps, pq, static_cast<double>(pv), 0.0, 0.0, 0.0};
                const double mine = wave_sum7(v, lane);  // lane 8c holds component c
                if ((lane & 7) == 0 && lane < 32) lds_part[cur - p0][wave][lane >> 3] = mine;
                touched |= 1u << (cur - p0);
                ps = 0.0; pq = 0.0; pn = 0; pv = 0;
            }
            cur = piece;
        }
        pn += ta.n; pv += ta.nv; ps += ta.s; pq += ta.q;
    };
    for (unsigned j = 0;; ++j) {
        if (t_lo + wave + kPersistWaves * j >= t_end) break;
        const u64 row = read_lane_u64(my_row, j);
        const unsigned meta = __builtin_amdgcn_readlane(my_meta, j), piece = meta & 0xffffu;
        const double* const base = a.amount + row;
        if (meta & kUnionTileWhole) {
            TileAcc ta;
            lean_tile<kNT>(base, static_cast<unsigned>(kDenseTileOrdinals), a.amount, lane, a.has_where, a.wmin, a.wmax, a.shift, ta);
            take(piece, ta);
#ifdef AQE_LEAN_STAMPS
            if (j == 0) LEAN_STAMP(2);
#endif
            continue;
        }
        // the tile owns the rows [vlo, vhi) and holds slots of one piece or of two adjacent ones: the same 16-byte loads, a
        // pair that leaves the rows never addressed (such a lane reads rows 0 and 1 of the view), an odd last row on its
        // own; both pieces' sums in one pass under row masks, then handed on (nothing of the tile is live across a flush)
        const unsigned vhi = (meta >> 16) & 0x7ffu, vlo = (meta >> 27) & 1u;
        Row2 v2[kTileUnroll];
        bool ok[kTileUnroll];
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const unsigned oi = 2u * static_cast<unsigned>(lane) + 128u * static_cast<unsigned>(k);
            ok[k] = oi + 1u < vhi;
            const Row2* const p = reinterpret_cast<const Row2*>(ok[k] ? base + oi : a.amount);
            if (kNT) {
                v2[k].x = __builtin_nontemporal_load(&p->x);
                v2[k].y = __builtin_nontemporal_load(&p->y);
            } else {
                v2[k] = *p;
            }
        }
        const double xo = (vhi & 1u) ? base[vhi - 1u] : 0.0;  // (wave-uniform)
        const u64 phi = U->piece_hi[piece];
        const bool two = phi - row < vhi;  // (wave-uniform) the next piece starts inside the tile
        const unsigned mid = two ? static_cast<unsigned>(phi - row) : vhi;
        const unsigned hi = two ? (U->piece_hi[piece + 1u] - row < vhi ? static_cast<unsigned>(U->piece_hi[piece + 1u] - row) : vhi) : vhi;
        TileAcc t0, t1;  // rows [vlo, mid) of the first piece, [mid, hi) of the second
        auto add = [&](double x, unsigned r, bool ld) {
            const bool i0 = ld && r >= vlo && r < mid, i1 = ld && r >= mid && r < hi;
            const bool w = !a.has_where || (x >= a.wmin && x <= a.wmax);
            const double d0 = i0 && w ? x - a.shift : 0.0, d1 = i1 && w ? x - a.shift : 0.0;
            t0.nv += i0 ? 1u : 0u; t0.n += i0 && w ? 1u : 0u; t0.s += d0; t0.q += d0 * d0;
            t1.nv += i1 ? 1u : 0u; t1.n += i1 && w ? 1u : 0u; t1.s += d1; t1.q += d1 * d1;
        };
#pragma unroll
        for (int k = 0; k < kTileUnroll; ++k) {
            const unsigned oi = 2u * static_cast<unsigned>(lane) + 128u * static_cast<unsigned>(k);
            add(v2[k].x, oi, ok[k]);
            add(v2[k].y, oi + 1u, ok[k]);
        }
        if (vhi & 1u) add(xo, vhi - 1u, lane == 0);  // the odd last row, folded by lane 0
        take(piece, t0);
        if (two) take(piece + 1u, t1);
#ifdef AQE_LEAN_STAMPS
        if (j == 0) LEAN_STAMP(2);
#endif
    }
    LEAN_STAMP(3);
    if (cur != ~0u) take(~0u, TileAcc{});  // (flushes the last piece)
    if (lane == 0) lds_mask[wave] = touched;
    if (head_stager && static_cast<unsigned>(lane) < sizeof(LeanUnion) / 8u) reinterpret_cast<u64*>(&lds_round[0][0])[lane] = head_word;
    if (head_stager && lane == 0) *lds_max_rounds = 0u;
    __syncthreads();

    // ---- the share's partial of every piece it holds slots of: data, drain, ticket (as lean_query) ----
    if (wave == 0) {
        unsigned m = 0;
#pragma unroll
        for (unsigned j = 0; j < kPersistWaves; ++j) m |= lds_mask[j];
        m = __builtin_amdgcn_readfirstlane(m);
        // lane 4 j + c sends component c of piece p0 + 16 g + j: sixteen pieces per store instruction
        static_assert(kUnionWgPieces % 16 == 0, "pieces in sets of sixteen");
#pragma unroll
        for (unsigned g = 0; g < kUnionWgPieces / 16; ++g) {
            if (((m >> (16u * g)) & 0xffffu) == 0u) continue;  // (wave-uniform)
            const unsigned j = 16u * g + (static_cast<unsigned>(lane) >> 2), c = static_cast<unsigned>(lane) & 3u;
            const unsigned e = static_cast<unsigned>(__shfl(static_cast<int>(my_entry), static_cast<int>(j), 64));
            if ((m >> j) & 1u) {
                double x[kPersistWaves];
#pragma unroll
                for (unsigned w = 0; w < kPersistWaves; ++w) x[w] = lds_part[j][w][c];
                double s = 0.0;
#pragma unroll
                for (unsigned w = 0; w < kPersistWaves; ++w) s += x[w];  // wave order
                __hip_atomic_store(a.partials + static_cast<size_t>(e) * 4u + c, s, AQE_RLX);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partials are out before the ticket is drawn
        LEAN_STAMP(5);
        if (lane == 0) s_last = lean_ticket(a.counter, bid, G);
        LEAN_STAMP(6);
    }
    __syncthreads();
    if (!s_last) return;

    // ---- the last workgroup folds.  ONE batch of loads: the partial list (an entry per thread), the pieces' and the
    //      targets' ranges, the incidence list (two per thread) and the tails of the first kUnionJudgeSlots members, back
    //      to back (two words per thread; a member past the last: zeros); staged in lds_part, the tails in registers
    //      until the sums are done.  Whoever holds a tail's first word — its `rounds` — raises the union's largest round
    //      count in LDS with it, and so does a thread per member beyond those: what the judges' row width follows ----
    const LeanUnion& H = *reinterpret_cast<const LeanUnion*>(&lds_round[0][0]);
    const unsigned i = threadIdx.x;
    static_assert(kUnionJudgeSlots * kLeanTailWords <= 2 * kPersistThreads, "the first members' tails: two words per thread");
    static_assert(offsetof(LeanTail, rounds) == 0, "a tail's first word holds its rounds (low half)");
    auto first_tail_word = [&](unsigned x) -> u64 {
        const unsigned m = x / kLeanTailWords;
        return m < kUnionJudgeSlots && m < nmem ? reinterpret_cast<const u64*>(&members[m].tail)[x - m * kLeanTailWords] : 0ull;
    };
    const u64 mt0 = first_tail_word(i), mt1 = first_tail_word(i + kPersistThreads);
    unsigned more_rounds = 0;
    for (unsigned m = kUnionJudgeSlots + i; m < nmem; m += kPersistThreads) more_rounds = max(more_rounds, members[m].tail.rounds);
    if (i % kLeanTailWords == 0u) more_rounds = max(more_rounds, static_cast<unsigned>(mt0));
    if ((i + kPersistThreads) % kLeanTailWords == 0u) more_rounds = max(more_rounds, static_cast<unsigned>(mt1));
    const unsigned nent = H.nentries, npc = H.npieces, ntg = H.ntargets, ninc = H.nincidences;
    double e4[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < nent) {
#pragma unroll
        for (int c = 0; c < 4; ++c) e4[c] = __hip_atomic_load(a.partials + static_cast<size_t>(i) * 4u + c, AQE_RLX);
    }
    // the target sums: thread i sums component i & 3 of target t0 + i / 4, in two turns of 256 targets (t0 = 0, 256)
    constexpr unsigned kTurn = kPersistThreads / 4;
    static_assert(2 * kUnionMaxRows <= 2 * kTurn, "two turns of targets");
    const unsigned tt0 = i >> 2, tt1 = tt0 + kTurn, tc = i & 3u;
    unsigned pb = 0, pe = 0, tb0 = 0, te0 = 0, tb1 = 0, te1 = 0, inc0 = 0, inc1 = 0;
    if (i < npc) { pb = H.piece_entry[i]; pe = H.piece_entry[i + 1u]; }
    if (tt0 < ntg) { tb0 = H.target_begin[tt0]; te0 = H.target_begin[tt0 + 1u]; }
    if (tt1 < ntg) { tb1 = H.target_begin[tt1]; te1 = H.target_begin[tt1 + 1u]; }
    if (i < ninc) inc0 = H.target_entry[i];
    if (i + kPersistThreads < ninc) inc1 = H.target_entry[i + kPersistThreads];
    // lds_part as one flat list: [0, 4 kUnionMaxEntries) the entries, then the incidences; later [0, 2048) the judging
    // waves' words — a tail and a result per slot, member m in slot m mod kUnionJudgeSlots — and [2048, 4096) the rows of
    // round totals
    double* const F = &lds_part[0][0][0];
    unsigned* const Finc = reinterpret_cast<unsigned*>(F + 4 * kUnionMaxEntries);
    double* const rows = F + 2048;
    u64* const Ftails = reinterpret_cast<u64*>(F);
    unsigned long long* const Fres = Ftails + kUnionJudgeSlots * kLeanTailWords;
    static_assert(4 * kUnionMaxEntries * sizeof(double) + kUnionMaxIncidences * sizeof(unsigned) <= sizeof(lds_part), "the fold's staging fits lds_part");
    static_assert(kUnionMaxIncidences <= 2 * kPersistThreads && kUnionMaxEntries <= kPersistThreads && kUnionMaxPieces <= kPersistThreads, "one batch of loads");
    static_assert(2048 + 8 * kUnionMaxRows <= kMaxPersistRounds * kPersistWaves * kVec && kUnionJudgeSlots * (kLeanTailWords + kLeanResWords) <= 2048, "rows beside the judging waves' words");
    if (i < nent) {
#pragma unroll
        for (int c = 0; c < 4; ++c) F[4u * i + c] = e4[c];
    }
    if (i < ninc) Finc[i] = inc0;
    if (i + kPersistThreads < ninc) Finc[i + kPersistThreads] = inc1;
    if (more_rounds) atomicMax(lds_max_rounds, more_rounds);  // (after the batch's last load is issued)
    __syncthreads();
    LEAN_STAMP_FOLD(3);
    // (the piece sums read kFoldBatch LDS entries at a time before adding them in order: one LDS round trip per batch)
    constexpr unsigned kFoldBatch = 4;
    if (i < npc) {  // a piece's partials, in workgroup order, into its first entry
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (unsigned e0 = pb; e0 < pe; e0 += kFoldBatch) {
            double x[kFoldBatch][4];
#pragma unroll
            for (unsigned u = 0; u < kFoldBatch; ++u) {
                const unsigned e = e0 + u < pe ? e0 + u : pb;
#pragma unroll
                for (int c = 0; c < 4; ++c) x[u][c] = F[4u * e + c];
            }
#pragma unroll
            for (unsigned u = 0; u < kFoldBatch; ++u) {
                if (e0 + u < pe) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) s4[c] += x[u][c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) F[4u * pb + c] = s4[c];
    }
    __syncthreads();
    LEAN_STAMP_FOLD(4);
    // A target's pieces, ascending, one component per thread.  A target may add a few hundred pieces: its chain of adds
    // is fixed (bit-reproducible), so what is cut is the LDS round trips around it — kTargetBatch values per trip, and
    // the trips pipelined: batch k + 1's values are on their way (x1, then x0 again) while batch k is added, the
    // incidences read a further batch ahead, so that the chain waits for LDS once, at its start.
    auto target_sum = [&](unsigned tb, unsigned te) {
        constexpr unsigned kTargetBatch = 8;  // two value buffers and the incidences: 5 words per entry of a batch
        double r = 0.0;
        if (tb >= te) return r;
        unsigned e[kTargetBatch];
        double x0[kTargetBatch], x1[kTargetBatch];
        auto incidences = [&](unsigned k) {
#pragma unroll
            for (unsigned u = 0; u < kTargetBatch; ++u) e[u] = Finc[k + u < te ? k + u : tb];
        };
        auto values = [&](double (&x)[kTargetBatch]) {
#pragma unroll
            for (unsigned u = 0; u < kTargetBatch; ++u) x[u] = F[4u * e[u] + tc];
        };
        auto add = [&](const double (&x)[kTargetBatch], unsigned k) {  // ascending, each add guarded
#pragma unroll
            for (unsigned u = 0; u < kTargetBatch; ++u) {
                if (k + u < te) r += x[u];
            }
        };
        incidences(tb);
        values(x0);
        incidences(tb + kTargetBatch);
        for (unsigned k0 = tb; k0 < te; k0 += 2u * kTargetBatch) {
            values(x1);
            incidences(k0 + 2u * kTargetBatch);
            add(x0, k0);
            values(x0);
            incidences(k0 + 3u * kTargetBatch);
            add(x1, k0 + kTargetBatch);
        }
        return r;
    };
    const double r0 = tt0 < ntg ? target_sum(tb0, te0) : 0.0;
    const double r1 = tt1 < ntg ? target_sum(tb1, te1) : 0.0;
    __syncthreads();
    // target 2 L + g: group g of row L — (n, S, Q) at 3 g, its rows visited at 6 + g
    auto put = [&](unsigned t, double r) { rows[static_cast<size_t>(t >> 1) * 8u + (tc < 3u ? 3u * (t & 1u) + tc : 6u + (t & 1u))] = r; };
    if (tt0 < ntg) put(tt0, r0);
    if (tt1 < ntg) put(tt1, r1);
    if (i < kUnionJudgeSlots * kLeanTailWords) Ftails[i] = mt0;  // (the sums are done: the first members' tails take their slots)
    if (i + kPersistThreads < kUnionJudgeSlots * kLeanTailWords) Ftails[i + kPersistThreads] = mt1;
    __syncthreads();
    LEAN_STAMP_FOLD(5);
    // The judges (lean_union_judge), rows as wide as the union's largest round count asks for: the bench's members have 5
    // rounds — eight of them to a wave, one wave per SIMD, ONE pass for its 32.
    static_assert(kMaxPersistRounds <= 32, "a member's rounds fit a half wave");
    const unsigned max_rounds = *lds_max_rounds;  // (uniform)
    if (max_rounds <= 8u) lean_union_judge<8>(members, nmem, wave, lane, rows, Ftails, Fres, epoch);
    else if (max_rounds <= 16u) lean_union_judge<16>(members, nmem, wave, lane, rows, Ftails, Fres, epoch);
    else lean_union_judge<32>(members, nmem, wave, lane, rows, Ftails, Fres, epoch);
}

// One query on the workgroups bid = 0 .. G-1 (a launch of its own, or one group of a batch's launch).  `a`: the fields
// the sweep needs, in registers; K: the descriptor (the kernel arguments of a single launch, the batch's table in device
// memory otherwise) — read twice: a lane's two runs, and the tail.  A batch's sweep class (plans.hip, build_multi):
// members[0 .. nmem) are the descriptors of the queries that share this sweep, members[0] being K's; the sweep, the
// partial list and the ticket are the first one's, and the folding workgroup judges every member (wave m: members m,
// m + 16, ...) on the same round totals.  A launch of its own: nmem = 1.
template <bool kNT, bool kWide>
__device__ __forceinline__ void lean_query(const LeanLaunch& a, const LeanRuns* const runs, const LeanKarg K, const LeanLaunch* const members, const unsigned nmem,
                                           const unsigned bid, const unsigned G, const unsigned long long epoch,
                                           const LeanUnion* const uni = nullptr) {
    // a wave's sums of a round (zero where it swept none); in the folding workgroup, later, the launch's whole partial list
    __shared__ double lds_part[kMaxPersistRounds][kPersistWaves][kVec];
    static_assert(kMaxPersistRounds * kPersistWaves >= kLeanMaxSlots, "the partial list fits where the workgroup's own sums were");
    __shared__ double lds_round[kMaxPersistRounds][kVec];
    __shared__ unsigned lds_slot[kMaxPersistRounds];
    __shared__ unsigned lds_mask[kPersistWaves];  // rounds a wave swept tiles of
    __shared__ u64 lds_tail[64];
    __shared__ int s_last;
    if (uni) {  // a union group of a batch: the same LDS, another sweep and fold
        lean_union<kNT>(a, uni, members, nmem, bid, G, epoch, lds_part, lds_round, lds_mask, s_last);
        return;
    }
    const int lane = threadIdx.x & 63;
    const unsigned wave = threadIdx.x >> 6;
    LEAN_STAMP(0);
    // the run table: lane i holds runs i and i + 64.  One batch of loads, in flight while LDS is cleared.
    // (wide plans: the table goes to LDS instead, one copy per workgroup, and a tile's run is found by bisection)
    __shared__ u64 lds_row0[kWide ? kLeanWideRuns : 1];
    __shared__ unsigned lds_tb[kWide ? kLeanWideRuns : 1], lds_rows[kWide ? kLeanWideRuns : 1], lds_meta[kWide ? kLeanWideRuns : 1], lds_rslot[kWide ? kLeanWideRuns : 1];
    u64 my_row0 = 0, my_row0_hi = 0;
    unsigned my_tb = 0, my_rows = 0, my_meta = 0, my_slot = 0, my_tb_hi = 0, my_rows_hi = 0, my_meta_hi = 0, my_slot_hi = 0;
    if (kWide) {
        for (unsigned i = threadIdx.x; i < a.nruns; i += kPersistThreads) {
            lds_row0[i] = a.wide->row0[i]; lds_tb[i] = a.wide->tile_begin[i]; lds_rows[i] = a.wide->rows[i];
            lds_meta[i] = a.wide->meta[i]; lds_rslot[i] = a.wide->slot[i];
        }
        __syncthreads();
    } else {
        my_row0 = runs->row0[lane]; my_row0_hi = runs->row0[lane + 64];
        my_tb = runs->tile_begin[lane]; my_rows = runs->rows[lane]; my_meta = runs->meta[lane]; my_slot = runs->slot[lane];
        my_tb_hi = runs->tile_begin[lane + 64]; my_rows_hi = runs->rows[lane + 64]; my_meta_hi = runs->meta[lane + 64]; my_slot_hi = runs->slot[lane + 64];
    }
    // The tail of the descriptor — what only the folding workgroup reads — is fetched NOW, by the last wave, one word per
    // lane, and parked in LDS after the sweep: nobody knows yet who will fold, and whoever does must not start fetching
    // descriptor words then, one dependent round trip after the other.
    const bool stager = wave == kPersistWaves - 1u;
    u64 tail_word = 0;
    if (stager && static_cast<unsigned>(lane) < sizeof(LeanTail) / 8u) tail_word = reinterpret_cast<const AQE_KARG u64*>(&K->tail)[lane];
    // every wave clears its own rows of lds_part: nothing to wait for before the sweep
#pragma unroll
    for (unsigned i = 0; i < kMaxPersistRounds * kVec / 64; ++i) {
        const unsigned x = static_cast<unsigned>(lane) + 64u * i;
        lds_part[x >> 3][wave][x & 7u] = 0.0;
    }
    if (a.tail.want_ticks && bid == 0 && threadIdx.x == 0)
        __hip_atomic_store(lean_t0_word(a.counter), static_cast<u64>(__builtin_amdgcn_s_memrealtime()), AQE_RLX);
#ifdef AQE_LEAN_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    LEAN_STAMP(1);
#endif

    // Tiles: a contiguous share per workgroup (its wave j takes the j-th, (j + 16)-th, ... of them: the 16 waves stream one
    // window of the column, and the share holds tiles of one round or of a few consecutive ones) — or, for a plan of ONE
    // round, dealt out wave by wave across the launch (tile t to wave t mod 16 G: every HBM channel busy from the start)
    const bool dealt = a.tiles_per_wg == 0u;
    const unsigned t_lo = dealt ? bid * kPersistWaves : bid * a.tiles_per_wg;
    const unsigned t_end = dealt ? a.ntiles : (t_lo + a.tiles_per_wg < a.ntiles ? t_lo + a.tiles_per_wg : a.ntiles);
    const unsigned t_step = dealt ? G * kPersistWaves : kPersistWaves;
    Acc acc;
    unsigned cur = ~0u, cur_slot = 0, touched = 0;  // the round this wave is in; the rounds it has been in
    auto flush = [&]() {
        const double v[7] = {static_cast<double>(acc.na), acc.sa, acc.qa, static_cast<double>(acc.nb), acc.sb, acc.qb, static_cast<double>(acc.nv)};
        const double mine = wave_sum7(v, lane);  // lane 8c holds component c
        if ((lane & 7) == 0 && lane < 56) lds_part[cur][wave][lane >> 3] = mine;
        if (lane == 0) lds_slot[cur] = cur_slot;
        touched |= 1u << cur;
    };
    for (unsigned t = __builtin_amdgcn_readfirstlane(t_lo + wave); t < t_end; t += t_step) {
        // the run that owns tile t: the last whose first tile is <= t (ascending; 0xffffffff past the table)
        unsigned meta, run_slot, run_tb, run_rows, first;
        u64 run_row0;
        if (kWide) {
            unsigned lo = 0, hi = a.nruns;
            while (hi - lo > 1u) {
                const unsigned mid = (lo + hi) >> 1;
                if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(lds_tb[mid])) <= t) lo = mid; else hi = mid;
            }
            meta = __builtin_amdgcn_readfirstlane(lds_meta[lo]); run_slot = __builtin_amdgcn_readfirstlane(lds_rslot[lo]);
            run_tb = __builtin_amdgcn_readfirstlane(lds_tb[lo]); run_rows = __builtin_amdgcn_readfirstlane(lds_rows[lo]);
            run_row0 = uniform64(lds_row0[lo]);
            first = (t - run_tb) * static_cast<unsigned>(kDenseTileOrdinals);
        } else {
            const unsigned below = static_cast<unsigned>(__builtin_popcountll(__ballot(my_tb <= t))) + static_cast<unsigned>(__builtin_popcountll(__ballot(my_tb_hi <= t)));
            const bool hi = below > 64u;           // wave-uniform: the run sits in the lanes' second set
            const unsigned i = (below - 1u) & 63u;
            meta = hi ? __builtin_amdgcn_readlane(my_meta_hi, i) : __builtin_amdgcn_readlane(my_meta, i);
            run_slot = hi ? __builtin_amdgcn_readlane(my_slot_hi, i) : __builtin_amdgcn_readlane(my_slot, i);
            run_tb = hi ? __builtin_amdgcn_readlane(my_tb_hi, i) : __builtin_amdgcn_readlane(my_tb, i);
            run_rows = hi ? __builtin_amdgcn_readlane(my_rows_hi, i) : __builtin_amdgcn_readlane(my_rows, i);
            run_row0 = hi ? read_lane_u64(my_row0_hi, i) : read_lane_u64(my_row0, i);
            first = (t - run_tb) * static_cast<unsigned>(kDenseTileOrdinals);
            if (meta & kLeanMetaSeg) {  // a row of equal blocks: the tile's block and its place in it (geometry in entry i + 64)
                const unsigned tps = __builtin_amdgcn_readlane(my_meta_hi, i), rel = t - run_tb;
                const unsigned blk = tps == 1u ? rel : rel / tps;
                run_row0 += static_cast<u64>(blk) * read_lane_u64(my_row0_hi, i);
                first = (rel - blk * tps) * static_cast<unsigned>(kDenseTileOrdinals);
            }
        }
        const unsigned r = meta & 0xffu;
        if (r != cur) {
            if (cur != ~0u) { flush(); acc = Acc{}; }
            cur = r;
            cur_slot = run_slot;
        }
        const unsigned rem = run_rows - first;
        const double* const base = a.amount + (run_row0 + first);
        TileAcc ta;
#ifndef AQE_ABL_NOSWEEP  // (ablation builds, tools/ab_ablate.sh: what each stage of a launch costs; results are then wrong)
        lean_tile<kNT>(base, rem, a.amount, lane, a.has_where, a.wmin, a.wmax, a.shift, ta);
#else
        ta.s = static_cast<double>(reinterpret_cast<uintptr_t>(base) & 1u) + rem;
#endif
        merge_tile(acc, ta, (meta & kLeanMetaGroupB) != 0);
#ifdef AQE_LEAN_STAMPS
        if (t == t_lo + wave) LEAN_STAMP(2);
#endif
    }
    LEAN_STAMP(3);
    if (cur != ~0u) flush();
    if (lane == 0) lds_mask[wave] = touched;
    if (stager) lds_tail[lane] = tail_word;
    LEAN_STAMP(4);
    __syncthreads();
#ifdef AQE_ABL_NOTICKET
    return;
#endif

    // ---- the workgroup's partial of every round it swept tiles of: data, drain, ticket (cdna_hip_programming.md G16) ----
    if (wave == 0) {
        unsigned m = 0;
#pragma unroll
        for (unsigned j = 0; j < kPersistWaves; ++j) m |= lds_mask[j];
        m = __builtin_amdgcn_readfirstlane(m);
        while (m) {
            const unsigned r = static_cast<unsigned>(__builtin_ctz(m));
            m &= m - 1u;
            const unsigned info = lds_slot[r];
            const unsigned slot = (info & 0xffffu) + bid - (info >> 16);  // the round's workgroups are consecutive
            if (lane < 7) {
                double x[kPersistWaves];
#pragma unroll
                for (unsigned j = 0; j < kPersistWaves; ++j) x[j] = lds_part[r][j][lane];  // all reads in flight at once
                double s = 0.0;
#pragma unroll
                for (unsigned j = 0; j < kPersistWaves; ++j) s += x[j];  // wave order
                __hip_atomic_store(a.partials + static_cast<size_t>(slot) * kVec + lane, s, AQE_RLX);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partials are out before the ticket is drawn
        LEAN_STAMP(5);
        if (lane == 0) s_last = lean_ticket(a.counter, bid, G);
        LEAN_STAMP(6);
    }
    __syncthreads();
    if (!s_last) return;
#ifdef AQE_ABL_NOFOLD
    return;
#endif

    // ---- the last workgroup to arrive folds the launch.  Everything it needs from the descriptor is in LDS already.  The
    //      whole partial list — fewer than workgroups + rounds slots, whatever the size of the sweep — is fetched in ONE batch
    //      of coalesced loads (three words per thread at most) into the space the workgroup's own sums occupied ----
    const LeanTail& T = *reinterpret_cast<const LeanTail*>(lds_tail);
    const unsigned rounds = T.rounds;
    // the other members' tails (wave m < 16 fetches member m's, one word per lane): in flight beside the partial list
    constexpr unsigned kTailWords = sizeof(LeanTail) / 8u;
    u64 mtail = 0;
    if (wave != 0 && wave < nmem && static_cast<unsigned>(lane) < kTailWords) mtail = reinterpret_cast<const u64*>(&members[wave].tail)[lane];
    const unsigned long long t0 = T.want_ticks ? __hip_atomic_load(lean_t0_word(a.counter), AQE_RLX) : 0ull;  // (in flight beside the partials)
    // W waves per round (a power of two; one when the plan has more than eight rounds).  Thread (part, c) of a round's waves
    // sums component c of every (8 W)-th slot of the round straight out of the partial list — fewer than workgroups + rounds
    // slots, whatever the size of the sweep: all of a thread's loads in flight together, ONE round trip for the launch — in
    // ascending order; the eight parts of a wave combine by DPP, the W waves of a round through LDS, in wave order: a fixed
    // order whatever arrives when — bit-reproducible.
#ifdef AQE_ABL_FOLD0  // (ablation: the folding workgroup stops here — tail in LDS read, nothing fetched yet)
    if (rounds != 0x7fffffffu) return;
#endif
    unsigned W = 1;
    while (2u * W * rounds <= kPersistWaves) W *= 2u;
    const unsigned wshift = static_cast<unsigned>(__builtin_ctz(W)), per_pass = kPersistWaves >> wshift;
    for (unsigned q0 = 0; q0 < rounds; q0 += per_pass) {
        const unsigned q = q0 + (wave >> wshift), wsub = wave & (W - 1u);
        const unsigned c = (static_cast<unsigned>(lane) >> 3) & 7u, part = (static_cast<unsigned>(lane) & 7u) + 8u * wsub;
        const bool mine = q < rounds && c < 7u;
        const unsigned b = mine ? T.slot_begin[q] : 0u, e = mine ? T.slot_begin[q + 1u] : 0u;
        double s = 0.0;
        constexpr unsigned kInFlight = 6;  // covers a round of 96 W slots in one turn (a 10 M-row query's rounds: ~65 slots, W = 2)
        for (unsigned sl0 = b + part; __ballot(sl0 < e) != 0; sl0 += 8u * W * kInFlight) {
            double x[kInFlight];
#pragma unroll
            for (unsigned i = 0; i < kInFlight; ++i) {
                const unsigned sl = sl0 + 8u * W * i;
#ifndef AQE_ABL_NOGATHER
                x[i] = sl < e ? __hip_atomic_load(a.partials + static_cast<size_t>(sl) * kVec + c, AQE_RLX) : 0.0;
#else
                x[i] = 1.0;
#endif
            }
#pragma unroll
            for (unsigned i = 0; i < kInFlight; ++i) s += x[i];
        }
        s += dpp_f64<0xB1>(s);   // lane ^ 1
        s += dpp_f64<0x4E>(s);   // lane ^ 2
        s += dpp_f64<0x141>(s);  // the other quad of the eight
        if (mine && (lane & 7) == 0) lds_round[q * W + wsub][c] = s;
    }
#ifdef AQE_ABL_FOLD1  // (ablation: ... here — partials fetched and summed per round, before the barrier)
    if (rounds != 0x7fffffffu) return;
#endif
    __syncthreads();
    LEAN_STAMP_FOLD(1);
    if (wave >= nmem) return;
#ifdef AQE_ABL_FOLD2  // (ablation: ... here — after the barrier, before the scan and the rules)
    if (rounds != 0x7fffffffu) return;
#endif
    // A judging wave's LDS: a member's tail (64 words) and the finishing lane's result, word by word (lean_send_result) —
    // in lds_part, which nobody reads after the ticket.  Member 0's tail is T.
    static_assert(kPersistWaves * 128 * sizeof(u64) <= sizeof(lds_part), "the judging waves' words fit in lds_part");
    u64* const lds_mine = reinterpret_cast<u64*>(&lds_part[0][0][0]) + wave * 128u;
    unsigned long long* const lds_res = lds_mine + 64;
    if (wave != 0) { lds_mine[lane] = mtail; wave_lds_handoff(); }
    // lane q: the moments through round q (a slot's own total in the totals form, and for the top-up slot).  The members of
    // a class agree on rounds, top-up slot and form: every judging wave scans the same rows the same way.
    const bool tslot = T.topup_slot != 0;
    const bool own = T.totals_only != 0 || (tslot && static_cast<unsigned>(lane) == rounds - 1u);
    // Row L of lds_round (round-major, the W waves of a round in wave order; at most 32 rows) goes to lane L — ONE batch of
    // LDS reads — and the rounds are scanned ACROSS the lanes with DPP shifts: an inclusive prefix over the rows (what the
    // rules judge: the moments through round q) and, beside it, every round's own total (the totals form; the top-up slot).
    // The loop this replaces — every lane walking all rows, one LDS round trip after the other — was 1.4 us of a 10 us
    // launch (profiles/round3_lean_ablation.txt).  Fixed shift pattern: bit-reproducible.
    for (unsigned mi = wave;;) {  // (the scan is redone per member: nothing lives across the judges)
        double tot[7];
        {
            const unsigned nrow = rounds * W;
            double own_t[7];
#pragma unroll
            for (int cc = 0; cc < 7; ++cc) tot[cc] = static_cast<unsigned>(lane) < nrow ? lds_round[lane][cc] : 0.0;
#pragma unroll
            for (int cc = 0; cc < 7; ++cc) {
                double o = tot[cc];  // the W rows of a round: aligned groups of W lanes (W = 1, 2, 4, 8 or 16), butterfly
                if (W >= 2u) o += dpp_f64<0xB1>(o);    // lane ^ 1
                if (W >= 4u) o += dpp_f64<0x4E>(o);    // lane ^ 2
                if (W >= 8u) o += dpp_f64<0x141>(o);   // the other quad of the eight (all four of its lanes agree)
                if (W >= 16u) o += dpp_f64<0x128>(o);  // the other half of the row of sixteen
                own_t[cc] = o;
                double p = tot[cc];  // inclusive prefix within the row of sixteen: shifts by 1, 2, 4, 8 (lanes shifted in from outside add 0)
                p += dpp_f64<0x111>(p);
                p += dpp_f64<0x112>(p);
                p += dpp_f64<0x114>(p);
                p += dpp_f64<0x118>(p);
                const double carry = read_lane_f64(p, 15);  // rows 16 .. 31 sit in the second row of lanes: plus the first row's total
                tot[cc] = p + (lane >= 16 ? carry : 0.0);
            }
            if (W > 1u) {  // lane q takes what the last row of round q holds
                const int src = static_cast<int>((static_cast<unsigned>(lane) + 1u) * W - 1u) & 63;
#pragma unroll
                for (int cc = 0; cc < 7; ++cc) { tot[cc] = __shfl(tot[cc], src, 64); own_t[cc] = __shfl(own_t[cc], src, 64); }
            }
#pragma unroll
            for (int cc = 0; cc < 7; ++cc) tot[cc] = own ? own_t[cc] : tot[cc];
        }
#ifdef AQE_ABL_FOLD3  // (ablation: ... here — rounds scanned, nothing judged or stored)
        if (tot[0] + tot[6] != -1.0) { if (lane == 0) T.state->n_a = tot[0] + tot[1] + tot[2] + tot[3] + tot[4] + tot[5] + tot[6]; return; }
#endif
        const LeanTail& Tm = mi == 0 ? T : *reinterpret_cast<const LeanTail*>(lds_mine);
        lean_judge(Tm, tot, static_cast<unsigned>(lane), t0, epoch, lds_res);
        wave_lds_handoff();  // (the finishing lane's words, read by the whole wave)
        lean_send_result(Tm, lds_res, static_cast<unsigned>(lane));
        mi += kPersistWaves;
        if (mi >= nmem) break;
        // a class of more than 16 members: this wave's next one (its tail is fetched now: one round trip)
        const u64 w = static_cast<unsigned>(lane) < kTailWords ? reinterpret_cast<const u64*>(&members[mi].tail)[lane] : 0ull;
        wave_lds_handoff();
        lds_mine[lane] = w;
        wave_lds_handoff();
    }
}

template <bool kNT, bool kWide>
__global__ __launch_bounds__(kPersistThreads) void k_sweep_lean(LeanLaunch a) {
    const LeanKarg K = (LeanKarg)__builtin_amdgcn_kernarg_segment_ptr();
    // (the run table is read out of the kernel-argument segment itself, per lane: ordinary global memory)
    lean_query<kNT, kWide>(a, &((const LeanLaunch*)K)->runs, K, nullptr, 1u, blockIdx.x, gridDim.x, a.epoch);
}

// A BATCH of queries in one launch (as k_sweep_multi, persist.hip): the grid is cut into one group of workgroups per
// sweep class, wg_map[blockIdx.x] = members << 48 | first member << 32 | group size << 16 | index in the group; group q
// runs table[q] exactly as a launch of its own would on that many workgroups, and judges table[q .. q + members) on its
// totals.  A group whose first descriptor names a union (`uni`) sweeps the union of several classes' runs instead and
// judges every member of them (lean_union).  Nothing here waits for anything — the last workgroup of a group to arrive
// finishes its queries — so groups may be dispatched in any order and there may be more of them than compute units.
template <bool kNT>
__global__ __launch_bounds__(kPersistThreads) void k_sweep_lean_multi(const LeanLaunch* table, const unsigned long long* wg_map, unsigned long long epoch) {
#ifdef AQE_LEAN_STAMPS
    {
        const int lane = threadIdx.x & 63;
        const unsigned wave = threadIdx.x >> 6;
        LEAN_STAMP(0);
    }
#endif
    const u64 me = uniform64(wg_map[blockIdx.x]);
    const unsigned q = static_cast<unsigned>(me >> 32) & 0xffffu, nmem = static_cast<unsigned>(me >> 48);
    const LeanKarg K = (LeanKarg)(table + q);
    LeanLaunch a;  // what the sweep reads, out of the table once
    a.amount = K->amount; a.ntiles = K->ntiles; a.tiles_per_wg = K->tiles_per_wg;
    a.has_where = K->has_where; a.wmin = K->wmin; a.wmax = K->wmax; a.shift = K->shift;
    a.partials = K->partials; a.counter = K->counter; a.tail.want_ticks = 0; a.wide = nullptr; a.nruns = 0;
    lean_query<kNT, false>(a, &(table + q)->runs, K, table + q, nmem, static_cast<unsigned>(me) & 0xffffu, static_cast<unsigned>(me >> 16) & 0xffffu, epoch,
                           K->uni);
}

}  // namespace

hipError_t launch_sweep_lean_multi(const LeanLaunch* table, const unsigned long long* wg_map, unsigned long long epoch, unsigned grid, bool nt,
                                   hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    if (nt) {
        if (ev0) hipExtLaunchKernelGGL(k_sweep_lean_multi<true>, dim3(grid), dim3(kPersistThreads), 0, s, ev0, ev1, 0, table, wg_map, epoch);
        else hipLaunchKernelGGL(k_sweep_lean_multi<true>, dim3(grid), dim3(kPersistThreads), 0, s, table, wg_map, epoch);
    } else {
        if (ev0) hipExtLaunchKernelGGL(k_sweep_lean_multi<false>, dim3(grid), dim3(kPersistThreads), 0, s, ev0, ev1, 0, table, wg_map, epoch);
        else hipLaunchKernelGGL(k_sweep_lean_multi<false>, dim3(grid), dim3(kPersistThreads), 0, s, table, wg_map, epoch);
    }
    return hipGetLastError();
}

hipError_t launch_sweep_lean(const LeanLaunch& a, unsigned grid, bool nt, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1) {
    auto go = [&](auto kernel) {
        if (ev0) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kPersistThreads), 0, s, ev0, ev1, 0, a);
        else hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPersistThreads), 0, s, a);
    };
    if (a.wide) { if (nt) go(k_sweep_lean<true, true>); else go(k_sweep_lean<false, true>); }
    else { if (nt) go(k_sweep_lean<true, false>); else go(k_sweep_lean<false, false>); }
    return hipGetLastError();
}

#ifdef AQE_LEAN_STAMPS
extern "C" __attribute__((visibility("default"))) int aqe_debug_lean_stamps(unsigned long long* out, size_t words) {
    const size_t all = LEAN_STAMP_BLOCKS * kLeanStampWords;  // (AQE_LEAN_STAMPS=2: the block of the even epochs, then the odd ones)
    return static_cast<int>(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lean_stamps), 8 * (words < all ? words : all), 0, hipMemcpyDeviceToHost));
}
#endif

}  // namespace aqe
