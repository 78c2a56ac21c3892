// Host side of the C ABI declared in include/ptq4vit_hip.h.
//
// Each *_calibrate entry point enqueues the complete calibration_step2() of one module on the
// caller's stream: interval initialisation, candidate tables, and for every search round the
// pack -> sweep -> finish -> select kernel chain for both operands.  Intervals live in device
// memory from start to end, so there is no host round trip inside a module (the reference moves
// x/out/grad host<->device on every search call, quant_layers/linear.py:461-464).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <thread>
#include <mutex>
#include <string>
#include <unordered_map>
#include <type_traits>
#include <vector>

#include "../../include/ptq4vit_hip.h"
#include "../../include/ptq4vit_hip_debug.h"
#include "p4v_kernels.h"

using namespace p4v;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(P4V_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define CHK(expr)              \
    do {                       \
        int r_ = (expr);       \
        if (r_ != 0) return r_; \
    } while (0)

inline long rup(long x, long m) { return (x + m - 1) / m * m; }
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Bump allocator over the caller's workspace.  With base == nullptr it only counts (dry run):
// *_workspace_bytes() runs the same planning code as *_calibrate().
// Test hooks of the arena (ptq4vit_hip_debug.h).  One switch: with the gap at 0 (production) no allocation moves and nothing is recorded.
//   g_arena_gap     p4v_debug_set_arena_gap: bytes left unused behind every allocation, in the dry run as well
//   g_arena_ranges  p4v_debug_arena_ranges: while the gap is on, the merged [begin, end) byte ranges every allocation of the calling
//                   thread's last non-dry call covered (host side only; a rewind of `off` does not erase a range)
constexpr size_t WS_ALIGN = 16;            // minimum alignment of d_workspace (dwordx4 / LDS-DMA loads of the planes carved from it)
std::atomic<size_t> g_arena_gap{0};
thread_local std::vector<std::pair<size_t, size_t>> g_arena_ranges;
inline void arena_note(size_t b, size_t e) {
    if (e <= b) return;
    auto& v = g_arena_ranges;
    auto it = v.begin();
    while (it != v.end() && it->second < b) ++it;            // first range that touches or follows [b, e)
    if (it == v.end() || it->first > e) { v.insert(it, {b, e}); return; }
    it->first = std::min(it->first, b);
    it->second = std::max(it->second, e);
    auto nx = it + 1;
    while (nx != v.end() && nx->first <= it->second) { it->second = std::max(it->second, nx->second); nx = v.erase(nx); }
}

struct Arena {
    char* base;
    size_t cap, off, peak;
    size_t top;   // bytes taken from the END of the buffer: live for the whole call (candidate-plane cache), while the
                  // bump region [0, off) is rewound after every pass
    bool dry;
    size_t gap;
    Arena(void* b, size_t c) : base((char*)b), cap(c & ~(size_t)255), off(0), peak(0), top(0), dry(b == nullptr),
                               gap(g_arena_gap.load(std::memory_order_relaxed)) {
        if (!dry) g_arena_ranges.clear();
    }
    template <typename T> T* get(size_t n) {
        off = (size_t)rup((long)off, 256);
        T* p = dry ? nullptr : (T*)(base + off);
        if (gap && !dry) arena_note(off, off + n * sizeof(T));
        off += n * sizeof(T) + gap;
        if (off + top > peak) peak = off + top;
        return p;
    }
    char* get_top(size_t bytes) {
        top += (size_t)rup((long)bytes, 256) + gap;           // (the gap lies behind the buffer, towards the end of the workspace)
        if (off + top > peak) peak = off + top;
        if (dry || top > cap) return nullptr;
        if (gap) arena_note(cap - top, cap - top + bytes);
        return base + cap - top;
    }
    bool ok() const { return dry || off + top <= cap; }
};
// gives back, at the end of its scope, what was taken from the bump region since (the peak keeps what it reached)
struct ArenaMark {
    Arena& a;
    const size_t off;
    explicit ArenaMark(Arena& a_) : a(a_), off(a_.off) {}
    ~ArenaMark() { a.off = off; }
};

// ---- optional per-launch timing of the sweep kernels (bench.py roofline) -----------------------
// Per CALLING THREAD: a thread that enabled timing (p4v_stats_enable) gets an event pair around every sweep launch
// it enqueues and reads its own totals back with p4v_stats_get.  Nothing here is shared between threads, so calls
// on other threads / streams / devices are unaffected.
struct StatRec { hipEvent_t a, b; int kind; double macs, alg; int stage, gx, gz; double ms, bytes; };
thread_local double g_alg_bytes = 0;       // compulsory bytes of the pass being launched: its fp32 operands + raw_out / raw_grad, once
thread_local double g_alg_macs_cand = 0;   // unpadded single-plane MACs of one candidate of the pass being launched
thread_local double g_exec_frac = 1.0;     // share of a launch's candidates that a pruned pass executes (stats mode only)
thread_local bool g_stat_on = false;
thread_local std::vector<StatRec> g_stat_recs;
thread_local std::vector<StatRec> g_stat_done;   // drained records, kept until p4v_stats_reset (p4v_stats_launches)
thread_local bool g_b1_keep = false;            // p4v_debug_bound_totals: keep the stage-B1 totals of this thread's pruned passes
thread_local std::vector<float> g_b1_totals;
// p4v_debug_prune_tables: keep the stage tables of this thread's pruned passes (keep_prune_tables: the record's layout).  A record
// is 32-bit words, the floats by their bits.  g_pass_round / g_pass_side: which pass of the call search_rounds is running (-1: none)
thread_local bool g_tables_keep = false;
thread_local std::vector<int32_t> g_tables;
thread_local int g_pass_round = -1, g_pass_side = -1;
// Which stage of a pruned pass is being launched: a label for the launch records and the prints, nothing decides by it.  Set by
// run_stage only (and cleared per call at the group entry); _lib.py maps the numbers to the record strings.
enum PruneStage { STAGE_FULL = 0, STAGE_A = 1, STAGE_B1 = 2, STAGE_B2 = 3, STAGE_A2 = 4 };   // A2: the second tier's slice sweep
thread_local int g_stage = STAGE_FULL;
thread_local p4v_kernel_stats g_stats = {};
thread_local long g_memo_hits = 0, g_memo_misses = 0;
// Process-wide counters of the exact candidate pruning (p4v_prune_counters): tests and bench.py assert with them that the
// three-stage passes -- not the full sweeps -- produced a result, whatever thread / stream the calibrator ran the module on.
//   [0] passes run in three stages   [1] ... whose stage B2 was empty (B1's candidates were the only survivors; host knew)
//   [2] prunable passes that ran the full sweep instead (slice too large / loose bounds / unsupported layout)
//   [3] passes not eligible at all (score tables requested, cosine, fp32 planes, pruning switched off)
std::atomic<long long> g_prune_cnt[4];
// Kernel-variant switches for A/B measurements and kernel-vs-kernel agreement tests (p4v_debug_set_variant; 0 in
// production).  One relaxed atomic word, read once per pass; every bit is a reference path a test or bench.py uses
// (paths that lost their measurement were removed together with their bits -- p4v_debug_set_variant rejects those):
//   1, 2: kernel debug flags (SweepParams::dbg)
//   4   no stationary-operand sweeps (everything on k_sweep2)
//   2048 cosine Linear searches on k_sweep2 (swapped operands, one GEMM per V block) instead of k_sweep6
//   32768 no k_sweep7 (K >= 1024 sweeps on k_sweep2 / k_sweep2g)      65536 no k_sweep8 (single-k-tile sweeps on k_sweep2)
//   131072 no k_sos_split      524288 no k_sweep9      1048576 k_sweep9 wherever it applies (not only on padded tiles)
//   2097152 post-GELU twin of k_sweep7 on two streamed planes (not the merged one)
//   4194304 no exact candidate pruning (every candidate over every sample)   8388608 prune even where the slice's bounds are loose
//   134217728 cross-check: every pruned pass is followed by the full sweep of the same pass, a differing selection is an error
//   bit 30: route every int8 sweep through the generic k_sweep
constexpr int VARIANT_KEPT = 1 | 2 | 4 | 2048 | 32768 | 65536 | 131072 | 524288 | 1048576 | 2097152 | 4194304 | 8388608 | 134217728;
std::atomic<int> g_variant_word{0};
#define g_variant (g_variant_word.load(std::memory_order_relaxed) & 0x3fffffff)
#define g_force_v1 ((g_variant_word.load(std::memory_order_relaxed) >> 30) & 1)
// tuning overrides of the launch heuristics (p4v_debug_set_tuning; <= 0: use the cost model)
std::atomic<int> g_tune[16];
enum { TUNE_CG6 = 0, TUNE_CG2 = 1, TUNE_CG2G = 2, TUNE_CG7 = 3, TUNE_PRINT = 4, TUNE_ORDER7 = 5, TUNE_P6 = 6, TUNE_PLANE_GIB = 7, TUNE_EPI6W = 8,
       TUNE_LOOSE_PCT = 9, TUNE_SLICE_DIV = 10, TUNE_SLICE_SMALL = 11, TUNE_B1_PATH = 12, TUNE_TIER2 = 13, TUNE_TIER2_DIV = 14, TUNE_LOOSE_ROWS = 15 };   // LOOSE_ROWS: sample rows from which a module prunes on a 5 % slice share   // TIER2: 1 = no second slice tier; >= 2: minimum survivor count that triggers it   // SLICE_SMALL: rows of the slice a Linear tries first   // pruning: weight share below which a module keeps full sweeps (%); Linear slice = M / div   // EPI6W: 1 = fragment-order epilogue image also in the weight search   // P6: k_sweep6 prologue, 0.1 us; PLANE_GIB: plane budget per chunk (cache limit = half)
// TUNE_B1_PATH (key 12) doubles as the switch of the reference paths the tests use: 7 cosine on the generic kernel, 9 no
// per-score-block candidate ranges, 11 quant_fast1 instead of quant16_sat8, >= 16 k_bound timing ablations, 4 the previous
// stage-B1 kernel of Linear passes (k_bound with a 64 x 32 wave tile: the before / after handle of the tests and of the timing).
// Values 1, 2, 3, 5, 6, 8, 10 and 12 selected paths that were measured and removed; p4v_debug_set_tuning rejects them.
inline bool tune_b1_removed(int v) { return v == 1 || v == 2 || v == 3 || v == 5 || v == 6 || v == 8 || v == 10 || v == 12; }
inline int tune(int k) { return g_tune[k].load(std::memory_order_relaxed); }
inline bool b1_previous() { return tune(TUNE_B1_PATH) == 4; }

// Every entry point that takes a workspace refuses a pointer below the documented alignment before anything is launched.
inline int ws_aligned(const void* p) {
    return ((uintptr_t)p % WS_ALIGN) == 0 ? 0 : fail(P4V_ERR_INVALID, "d_workspace must be aligned to %zu bytes", WS_ALIGN);
}

struct Group;
struct Ctx {
    hipStream_t st;
    Arena ws;
    bool dry;
    Group* grp = nullptr;     // p4v_calibrate_group: this call is member `slot` of a group whose stream operations are deferred and
    int slot = 0;             // issued together (grouped launches); nullptr: every operation goes to `st` at once
    int par = 1;              // members of the group that search in lock step: the launch heuristics plan for 256 / par CUs
    // a real call on the caller's stream and workspace / the dry run of the planner behind *_workspace_bytes: it carves nothing,
    // launches nothing and counts; every tensor of its record is null
    static Ctx on(void* stream, void* workspace, size_t bytes) { return Ctx{(hipStream_t)stream, Arena(workspace, bytes), false}; }
    static Ctx sizing() { return Ctx{nullptr, Arena(nullptr, 0), true}; }
    size_t sized_bytes() const { return ws.peak + 4096; }     // what a sizing run reports
};

// ---- stream operations: issued at once (one module) or deferred and grouped (p4v_calibrate_group) -------------------------------
// Every kernel launch, fill and copy of the calibration path goes through enqueue() / q_fill() / q_d2h() / q_h2d() / q_sync().
// Without a group they act on c.st immediately.  With one, the operations of a member are queued in its own FIFO and the member
// runs ahead until it needs a result on the host (q_sync: the survivor range of a pruned pass, an interval for the pass memo);
// when every member of the group waits (or has finished), the last one to arrive merges the FIFOs -- repeatedly taking the most
// common head operation over all members and issuing those launches as ONE grouped launch (k_x_g) -- synchronises the stream
// once and releases everybody.  The members' operations never depend on each other (separate modules, separate scratch), every
// member's own order is kept, and a grouped launch runs each member's body on its own parameters: bit-identical results.
struct StatInfo { int kind; double macs, alg; int stage, gx, gz; double bytes; };   // a timed sweep launch (bench.py roofline)
struct QOp;
struct KernelDesc {
    hipError_t (*one)(const QOp&, hipStream_t);
    hipError_t (*many)(const QOp* const*, int, hipStream_t);   // nullptr: the kernel has no grouped entry point
    int cap;                                                    // members per grouped launch
};
constexpr int QOP_PARAM_BYTES = 480;
struct QOp {
    enum Type : int { KERNEL, FILL, D2H, H2D, COPY2D, WAIT };
    int type = KERNEL;
    const KernelDesc* kd = nullptr;
    dim3 grid, block;
    unsigned lds = 0;
    alignas(16) char params[QOP_PARAM_BYTES];
    void* dst = nullptr; const void* src = nullptr; size_t bytes = 0; int value = 0;
    size_t dpitch = 0, spitch = 0, width = 0, height = 0;
    std::vector<char> payload;      // H2D: the host data (the caller's buffer may be gone when the operation is issued)
    bool timed = false;             // record the launch (bench.py roofline)
    bool heavy = false;             // a sweep: the issuer holds it back until no light operation is left at any member's head, so that
    StatInfo si{};                  // members that lag a few small launches behind join the same grouped launch
};
inline hipError_t lds_attr(const void* fn, unsigned lds, std::atomic<bool>& done) {
    if (lds <= 48 * 1024 || done.load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) done.store(true, std::memory_order_release);
    return e;
}
template <typename P, void (*K1)(P), void (*KG)(GroupArgs<P>)> struct Kern {
    static_assert(sizeof(P) <= QOP_PARAM_BYTES, "kernel parameter block larger than a queued operation holds");
    static hipError_t one(const QOp& op, hipStream_t st) {
        static std::atomic<bool> attr{false};
        if (hipError_t e = lds_attr((const void*)K1, op.lds, attr); e != hipSuccess) return e;
        P p;
        std::memcpy(&p, op.params, sizeof(P));
        void* args[] = {&p};
        return hipLaunchKernel((const void*)K1, op.grid, op.block, args, op.lds, st);
    }
    static hipError_t many(const QOp* const* ops, int n, hipStream_t st) {
        static std::atomic<bool> attr{false};
        GroupArgs<P> a;
        unsigned off = 0, lds = 0;
        a.n = n;
        for (int m = 0; m < n; ++m) {
            const QOp& op = *ops[m];
            a.off[m] = off; a.gx[m] = op.grid.x; a.gy[m] = op.grid.y; a.gz[m] = op.grid.z;
            std::memcpy(&a.p[m], op.params, sizeof(P));
            off += (unsigned)rup((long)op.grid.x * op.grid.y * op.grid.z, 8);
            lds = std::max(lds, op.lds);
        }
        a.off[n] = off;
        if (hipError_t e = lds_attr((const void*)KG, lds, attr); e != hipSuccess) return e;
        void* args[] = {&a};
        return hipLaunchKernel((const void*)KG, dim3(off), ops[0]->block, args, lds, st);
    }
    static const KernelDesc* desc() { static const KernelDesc d{&one, &many, GroupArgs<P>::CAP}; return &d; }
};
template <typename P, void (*K1)(P)> struct Kern1 {      // kernels off the grouped path (generic fallbacks, API helpers)
    static_assert(sizeof(P) <= QOP_PARAM_BYTES, "kernel parameter block larger than a queued operation holds");
    static hipError_t one(const QOp& op, hipStream_t st) {
        static std::atomic<bool> attr{false};
        if (hipError_t e = lds_attr((const void*)K1, op.lds, attr); e != hipSuccess) return e;
        P p;
        std::memcpy(&p, op.params, sizeof(P));
        void* args[] = {&p};
        return hipLaunchKernel((const void*)K1, op.grid, op.block, args, op.lds, st);
    }
    static const KernelDesc* desc() { static const KernelDesc d{&one, nullptr, 1}; return &d; }
};
#define KERN(P, NAME) (Kern<P, NAME, NAME##_g>::desc())
#define KERN_T(P, NAME, ...) (Kern<P, NAME<__VA_ARGS__>, NAME##_g<__VA_ARGS__>>::desc())
#define KERN1_T(P, NAME, ...) (Kern1<P, NAME<__VA_ARGS__>>::desc())

constexpr int MIR_SLOT = 2048, MIR_SLOTS = 3;
// header of a mirror block, in ints: [0,1] / [2,3] survivor ranges of the two tiers, [4] the slice's weight share, [16..79] /
// [80..143] the per-score-block ranges of the two tiers (<= MIR_BLK blocks: the heads of an attention matmul), then the interval slots
constexpr int MIR_HDR = 160, MIR_BLK = 32, MIR_R1 = 0, MIR_R2 = 2, MIR_RB1 = 16, MIR_RB2 = 80;
constexpr size_t MIRROR_BYTES = sizeof(int) * MIR_HDR + sizeof(float) * MIR_SLOT * MIR_SLOTS;
inline int* mirror_alloc() {
    void* p = nullptr;
    if (hipHostMalloc(&p, MIRROR_BYTES, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
    return (int*)p;
}

// The rendezvous of one p4v_calibrate_group call (see above).
struct Group {
    hipStream_t st = nullptr;
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::deque<QOp>> q;      // member FIFOs: written by the member while it runs, read by the issuer while every member is blocked
    std::vector<int> state;              // 0 running, 1 waiting in q_sync, 2 finished
    int blocked = 0;
    unsigned long gen = 0;
    int status = 0;                      // first HIP error of an issue round (every waiting member returns it)
    std::string err;
    std::vector<int*> mirrors;           // one mapped host block per member (host_mirror)
    bool stat_on = false;
    std::vector<StatRec>* stat_recs = nullptr;      // the CALLING thread's launch records: one per grouped launch
    long n_ops = 0, n_launches = 0, n_rounds = 0;
    hipEvent_t inputs_ready = nullptr;   // the members' captured tensors are complete once this event has fired (nullptr: they are)
    bool waited = false;                 // ... and the stream already waits for it
    int last_par[16] = {};               // members in the last grouped launch of each sweep family (StatInfo.kind): what the members'
                                         // launch heuristics plan for (written by the issuer while every member is blocked)
    int issue_kernels(std::vector<const QOp*>& ops);
    int issue_round();                   // (mu held, every member blocked)
    int sync(int slot);
    void finish(int slot);
};

// Process-wide counters (p4v_launch_counters): [0] kernel launches the calibration path asked for (one module at a time these ARE
// the launches), [1] kernel launches issued to the GPU, [2] issue rounds of the groups, [3] group calls.
std::atomic<long long> g_launch_cnt[4];
int enqueue_now(hipStream_t st, const QOp& op, bool timed, std::vector<StatRec>* recs) {
    g_launch_cnt[1].fetch_add(1, std::memory_order_relaxed);
    StatRec rec{};
    if (timed) {
        HIPCHK(hipEventCreate(&rec.a));
        HIPCHK(hipEventCreate(&rec.b));
        HIPCHK(hipEventRecord(rec.a, st));
    }
    HIPCHK(op.kd->one(op, st));
    if (timed) {
        HIPCHK(hipEventRecord(rec.b, st));
        rec.kind = op.si.kind; rec.macs = op.si.macs; rec.alg = op.si.alg; rec.stage = op.si.stage; rec.gx = op.si.gx; rec.gz = op.si.gz; rec.bytes = op.si.bytes;
        recs->push_back(rec);
    }
    return 0;
}
int issue_plain(hipStream_t st, const QOp& op) {
    switch (op.type) {
        case QOp::FILL: HIPCHK(hipMemsetAsync(op.dst, op.value, op.bytes, st)); break;
        case QOp::D2H: HIPCHK(hipMemcpyAsync(op.dst, op.src, op.bytes, hipMemcpyDeviceToHost, st)); break;
        case QOp::H2D: HIPCHK(hipMemcpyAsync(op.dst, op.payload.data(), op.bytes, hipMemcpyHostToDevice, st)); break;
        case QOp::COPY2D: HIPCHK(hipMemcpy2DAsync(op.dst, op.dpitch, op.src, op.spitch, op.width, op.height, hipMemcpyDeviceToDevice, st)); break;
        default: break;
    }
    return 0;
}
// one grouped launch per <= cap members of `ops` (all of one kernel entry point and block shape), in balanced chunks
int Group::issue_kernels(std::vector<const QOp*>& ops) {
    const KernelDesc* kd = ops[0]->kd;
    const int total = (int)ops.size();
    if (ops[0]->heavy && ops[0]->si.kind >= 0 && ops[0]->si.kind < 16) last_par[ops[0]->si.kind] = total;
    if (!kd->many || total == 1) {
        for (const QOp* op : ops) { CHK(enqueue_now(st, *op, op->timed && stat_recs, stat_recs)); ++n_launches; }
        return 0;
    }
    const int chunks = cdiv(total, kd->cap), per = cdiv(total, chunks);
    for (int i0 = 0; i0 < total; i0 += per) {
        const int m = std::min(per, total - i0);
        bool timed = stat_recs != nullptr;
        for (int i = 0; i < m; ++i) timed = timed && ops[i0 + i]->timed;
        StatRec rec{};
        if (timed) {
            HIPCHK(hipEventCreate(&rec.a));
            HIPCHK(hipEventCreate(&rec.b));
            HIPCHK(hipEventRecord(rec.a, st));
        }
        HIPCHK(kd->many(ops.data() + i0, m, st));
        g_launch_cnt[1].fetch_add(1, std::memory_order_relaxed);
        ++n_launches;
        if (timed) {      // ONE record per kernel launch (1:1 with a kernel trace): the members' work added up
            HIPCHK(hipEventRecord(rec.b, st));
            // (grid_x = the flat grid of the grouped launch -- every member's blocks, padded to a multiple of 8 --, as a kernel trace
            // shows it; grid_z = the number of members)
            const StatInfo& s0 = ops[i0]->si;
            rec.kind = s0.kind; rec.stage = s0.stage; rec.gz = m;
            for (int i = 0; i < m; ++i) {
                const QOp& o = *ops[i0 + i];
                rec.macs += o.si.macs; rec.alg += o.si.alg; rec.bytes += o.si.bytes;
                rec.gx += (int)rup((long)o.grid.x * o.grid.y * o.grid.z, 8);
            }
            stat_recs->push_back(rec);
        }
    }
    return 0;
}
int Group::issue_round() {
    ++n_rounds;
    g_launch_cnt[2].fetch_add(1, std::memory_order_relaxed);
    std::vector<const QOp*> bucket;
    for (;;) {
        // the most common head operation over the members (kernel entry point + block shape; plain operations go one by one);
        // light operations first: a sweep waits until every member that can still reach one has
        int best = -1, best_n = 0;
        bool best_heavy = true;
        int n_wait = 0, n_live = 0;
        for (int i = 0; i < n; ++i) {
            if (q[i].empty()) continue;
            ++n_live;
            const QOp& h = q[i].front();
            if (h.type == QOp::WAIT) { ++n_wait; continue; }                    // (last: see below)
            if (h.type != QOp::KERNEL) { best = i; best_n = 0; break; }        // fills / copies: at once, in member order
            if (h.heavy && !best_heavy) continue;
            int cnt = 0;
            for (int j = i; j < n; ++j)
                if (!q[j].empty()) { const QOp& o = q[j].front(); cnt += o.type == QOp::KERNEL && o.kd == h.kd && o.block.x == h.block.x && o.block.y == h.block.y && o.block.z == h.block.z; }
            if ((best_heavy && !h.heavy) || cnt > best_n) { best = i; best_n = cnt; best_heavy = h.heavy; }
        }
        if (best < 0 && n_wait > 0) {
            // Every member that still has work stands before the point where it needs its captured tensors: only now does the
            // stream wait for the capture -- what the members queued before (weight abs-max, candidate tables, the candidate
            // planes of the weights) ran while the capture passes were still on the GPU.
            if (!waited && inputs_ready) { HIPCHK(hipStreamWaitEvent(st, inputs_ready, 0)); waited = true; }
            for (int i = 0; i < n; ++i)
                if (!q[i].empty() && q[i].front().type == QOp::WAIT) q[i].pop_front();
            continue;
        }
        if (best < 0) break;
        const QOp& h = q[best].front();
        if (h.type != QOp::KERNEL) {
            const int r = issue_plain(st, h);
            ++n_ops;
            q[best].pop_front();
            if (r) return r;
            continue;
        }
        bucket.clear();
        std::vector<int> who;
        for (int j = best; j < n; ++j)
            if (!q[j].empty()) { const QOp& o = q[j].front(); if (o.type == QOp::KERNEL && o.kd == h.kd && o.block.x == h.block.x && o.block.y == h.block.y && o.block.z == h.block.z) { bucket.push_back(&o); who.push_back(j); } }
        n_ops += (long)bucket.size();
        const int r = issue_kernels(bucket);
        for (int j : who) q[j].pop_front();
        if (r) return r;
    }
    return 0;
}
int Group::sync(int slot) {
    std::unique_lock<std::mutex> lk(mu);
    state[slot] = 1;
    ++blocked;
    if (blocked == n) {
        int r = issue_round();
        if (!r && hipStreamSynchronize(st) != hipSuccess) r = fail(P4V_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
        if (r && !status) { status = r; err = g_err; }
        blocked = 0;
        for (int i = 0; i < n; ++i) { if (state[i] == 1) state[i] = 0; else if (state[i] == 2) ++blocked; }
        ++gen;
        cv.notify_all();
    } else {
        const unsigned long g = gen;
        cv.wait(lk, [&] { return gen != g; });
    }
    if (status) { g_err = err; return status; }
    return 0;
}
void Group::finish(int slot) {
    std::unique_lock<std::mutex> lk(mu);
    state[slot] = 2;
    ++blocked;
    if (blocked < n) return;
    bool waiting = false;
    for (int i = 0; i < n; ++i) waiting = waiting || state[i] == 1;
    int r = issue_round();
    if (!r && waiting && hipStreamSynchronize(st) != hipSuccess) r = fail(P4V_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
    if (r && !status) { status = r; err = g_err; }
    blocked = 0;
    for (int i = 0; i < n; ++i) { if (state[i] == 1) state[i] = 0; else if (state[i] == 2) ++blocked; }
    ++gen;
    cv.notify_all();
}

// a kernel launch of the calibration path; `si`: the launch is one of the timed sweeps (roofline records)
template <typename P> int enqueue(Ctx& c, const KernelDesc* kd, dim3 grid, dim3 block, size_t lds, const P& p, const StatInfo* si = nullptr) {
    if (c.dry) return 0;
    QOp op;
    op.type = QOp::KERNEL; op.kd = kd; op.grid = grid; op.block = block; op.lds = (unsigned)lds;
    static_assert(sizeof(P) <= QOP_PARAM_BYTES, "parameter block too large");
    std::memcpy(op.params, &p, sizeof(P));
    if (si) { op.heavy = true; op.timed = g_stat_on; op.si = *si; }
    g_launch_cnt[0].fetch_add(1, std::memory_order_relaxed);
    if (c.grp) { c.grp->q[c.slot].push_back(std::move(op)); return 0; }
    return enqueue_now(c.st, op, op.timed, &g_stat_recs);
}
int q_fill(Ctx& c, void* dst, int value, size_t bytes) {        // (k_fill_bytes: a kernel of this library, so that fills join the grouped launches)
    if (c.dry || bytes == 0) return 0;
    const FillBytesParams p{dst, value, (long)bytes};
    const long items = (bytes & 3) == 0 ? (long)(bytes >> 2) : (long)bytes;
    return enqueue(c, KERN(FillBytesParams, k_fill_bytes), dim3((unsigned)std::min<long>(cdiv(items, 256), 2048)), dim3(256), 0, p, nullptr);
}
int q_d2h(Ctx& c, void* host, const void* dev, size_t bytes) {       // `host` must stay valid until the next q_sync
    if (!c.grp) { HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c.st)); return 0; }
    QOp op; op.type = QOp::D2H; op.dst = host; op.src = dev; op.bytes = bytes;
    c.grp->q[c.slot].push_back(std::move(op));
    return 0;
}
int q_h2d(Ctx& c, void* dev, const void* host, size_t bytes) {       // (callers synchronise before `host` goes away)
    if (!c.grp) { HIPCHK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c.st)); return 0; }
    QOp op; op.type = QOp::H2D; op.dst = dev; op.bytes = bytes;
    op.payload.assign((const char*)host, (const char*)host + bytes);
    c.grp->q[c.slot].push_back(std::move(op));
    return 0;
}
int q_copy2d(Ctx& c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height) {
    if (!c.grp) { HIPCHK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, c.st)); return 0; }
    QOp op; op.type = QOp::COPY2D; op.dst = dst; op.src = src; op.dpitch = dpitch; op.spitch = spitch; op.width = width; op.height = height;
    c.grp->q[c.slot].push_back(std::move(op));
    return 0;
}
// from here on the call reads its captured tensors (raw_input / raw_out / raw_grad): inside a group whose caller handed over a
// "capture done" event, the stream waits for it -- once, when every member has reached this point
int q_wait_inputs(Ctx& c) {
    if (c.dry || !c.grp || !c.grp->inputs_ready) return 0;
    QOp op; op.type = QOp::WAIT;
    c.grp->q[c.slot].push_back(std::move(op));
    return 0;
}
int q_sync(Ctx& c) {
    if (c.grp) return c.grp->sync(c.slot);
    HIPCHK(hipStreamSynchronize(c.st));
    return 0;
}

// Small device -> host results (the survivor range of a pruned pass, the slice's weight share, the intervals a pass selected)
// are written by their kernel into mapped host memory as well and read after the stream synchronisation the host does anyway:
// no copy command (a pageable hipMemcpyAsync is a blit kernel into a staging buffer between two waits: ~410 range read-backs
// and ~270 interval read-backs per ViT-B calibration).  One block per (device, stream) -- per MEMBER inside a group --, allocated
// at first use (the calibrator's streams are persistent), never freed: 32 ints ([0,1] / [2,3] survivor ranges of the two tiers,
// [4] weight share, [8..15] / [16..23] their per-score-block ranges) + MIR_SLOTS interval vectors of MIR_SLOT floats.  The null
// stream has no block (calls from different threads would share it): it takes the copy path, as does a stream whose allocation failed.
int* host_mirror(Ctx& c) {
    if (c.grp) return c.grp->mirrors[c.slot];
    if (!c.st) return nullptr;
    static std::mutex mu;
    static std::unordered_map<unsigned long long, int*> tab;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const unsigned long long key = (unsigned long long)(uintptr_t)c.st ^ ((unsigned long long)(dev + 1) << 56);
    std::lock_guard<std::mutex> lk(mu);
    auto it = tab.find(key);
    if (it != tab.end()) return it->second;
    int* p = mirror_alloc();
    tab[key] = p;
    return p;
}
// The interval vectors of the *_impl call running on this thread that are mirrored (MirrorScope binds them, launch_select /
// k_prune_hull write through attach_mirror, read_dev reads).  `valid`: the last writer of the whole device vector was a
// mirrored selection (not the min-max initialisation, not a memo restore).
struct IvMirror { const float* dev; float* host; bool valid; int count; };
thread_local IvMirror g_mir[MIR_SLOTS] = {};
IvMirror* mirror_of(const float* dev) {
    if (!dev) return nullptr;
    for (auto& m : g_mir) if (m.dev == dev) return &m;
    return nullptr;
}
void attach_mirror(SelectParams& sl) {
    sl.iv_host = nullptr; sl.aux_host = nullptr;
    // whatever this selection writes, the mirrors of its outputs are stale until it proves otherwise
    IvMirror* mi = mirror_of(sl.interval);
    IvMirror* ma = mirror_of(sl.aux_out);
    if (mi) mi->valid = false;
    if (ma) ma->valid = false;
    if (mi && sl.nj <= MIR_SLOT && sl.out_off == 0 && (sl.nj == 1 || sl.out_js == 1)) { sl.iv_host = mi->host; mi->valid = true; mi->count = sl.nj; }
    if (ma && sl.nj <= MIR_SLOT) { sl.aux_host = ma->host; ma->valid = true; ma->count = sl.nj; }
}

void metric_epi(int metric, int* epi, int* wt_mode) {
    switch (metric) {
        case P4V_METRIC_L1_NORM: *epi = EPI_ABS; *wt_mode = 0; break;
        case P4V_METRIC_L2_NORM: *epi = EPI_SQ; *wt_mode = 0; break;
        case P4V_METRIC_LINEAR_WEIGHTED_L2: *epi = EPI_W_SQ; *wt_mode = 3; break;
        case P4V_METRIC_SQUARE_WEIGHTED_L2: *epi = EPI_SQ_W; *wt_mode = 2; break;
        case P4V_METRIC_HESSIAN: *epi = EPI_SQ_W; *wt_mode = 1; break;
        default: *epi = EPI_COS; *wt_mode = 0; break;
    }
}

// The weight-source rule (include/ptq4vit_hip.h, d_grad): raw_grad is read if and only if the metric is hessian, as in the
// reference (linear.py:409-421).  Every *_impl takes its tensor record through this function, so Pass::G and the split job's
// kp.G are null under every other metric whatever the caller passed, and every `Wt = G ? G : O` below resolves to raw_out
// there.  That matters to the kernels that take the weight from the POINTER and not from wt_mode -- k_bound's epilogue reads
// Wt in place -- and to the host code that keys on it (slice_fill's gather of raw_grad rows, the conv's transposed copy).
template <typename Tensors> Tensors grad_by_metric(Tensors t, int metric) {
    int epi = 0, wt_mode = 0;
    metric_epi(metric, &epi, &wt_mode);
    if (wt_mode != 1) t.G = nullptr;
    return t;
}

// ---- launch helpers ---------------------------------------------------------------------------
// `empty_is_zero`: a block of nothing but padding decodes to 0 (the reference pads with zeros) -- the running maxima start at
// enc(+0.0f), the bit pattern of -0.0f, instead of at "nothing seen" (which decodes to NaN)
int launch_absmax(Ctx& c, const float* src, const long (&st)[4], int D0, int D1, int R, int C, int nV, int nH,
                  int crb_r, int crb_c, int signed_max, unsigned* out, bool empty_is_zero = false) {
    if (c.dry) return 0;
    const int n = D1 * nV * nH;
    if (empty_is_zero) CHK(enqueue(c, KERN(FillParams, k_fill_f32), dim3(cdiv(n, 256)), dim3(256), 0, FillParams{reinterpret_cast<float*>(out), -0.0f, n}));
    else CHK(q_fill(c, out, 0, sizeof(unsigned) * (size_t)n));  // 0 < enc(x) for every float x
    AbsMaxParams p{src, st[0], st[1], st[2], st[3], D0, D1, R, C, nV, nH, crb_r, crb_c, 0, signed_max, out};
    p.row_tile = std::max(1, std::min(crb_r, std::max(1, 8192 / std::max(1, std::min(crb_c, C)))));
    const int tiles_per_v = cdiv(crb_r, p.row_tile);
    dim3 grid(tiles_per_v * nV * nH, D1, D0);
    return enqueue(c, KERN(AbsMaxParams, k_absmax), grid, dim3(256), 0, p);
}

int launch_interval(Ctx& c, const unsigned* enc, int n, float denom, int broadcast, float* interval) {
    if (c.dry) return 0;
    return enqueue(c, KERN(IntervalParams, k_interval_from_max), dim3(cdiv(n, 64)), dim3(64), 0, IntervalParams{enc, n, denom, broadcast, interval});
}

int launch_cands(Ctx& c, const float* mult, const float* interval, int ncand, int nblk, float* cands) {
    if (c.dry) return 0;
    return enqueue(c, KERN(CandsParams, k_make_cands), dim3(cdiv((long)ncand * nblk, 256)), dim3(256), 0, CandsParams{mult, interval, ncand, nblk, cands});
}

int launch_scale(Ctx& c, ScaleParams p) {
    if (c.dry) return 0;
    return enqueue(c, KERN(ScaleParams, k_scale_table), dim3(cdiv((long)p.C * p.nblk, 256)), dim3(256), 0, p);
}

// The rounding of v_cvt_pk_u8_f32 (k_probe_cvt, once per process) -> the bias of quant16_sat8: 128.5 where the conversion
// truncates, 128 where it rounds to nearest; 0 = not usable (the kernels keep quant_fast1).  The probe writes 8 words of a
// scratch allocation of its own (never the caller's workspace or output), under a mutex, on the caller's stream; only a probe
// that RAN and returned unexpected values latches "unusable" -- a failed launch / copy / synchronisation (a capturing stream, ...)
// leaves the state unknown: this call keeps quant_fast1 and the next one probes again.
std::atomic<int> g_cvt_state{0};      // 0 unknown, 1 truncates, 2 rounds to nearest, 3 unusable
void cvt_probe(hipStream_t stream) {
    if (g_cvt_state.load(std::memory_order_acquire) != 0) return;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (g_cvt_state.load(std::memory_order_acquire) != 0) return;
    static unsigned* scratch = nullptr;
    if (!scratch && hipMalloc(&scratch, 8 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); scratch = nullptr; return; }
    unsigned h[5] = {9, 9, 9, 9, 9};
    hipLaunchKernelGGL(k_probe_cvt, dim3(1), dim3(64), 0, stream, scratch);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, scratch, sizeof h, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); return; }
    const bool sat = h[3] == 0 && h[4] == 255;
    const int st = (sat && h[0] == 0 && h[1] == 1 && h[2] == 2) ? 1 : (sat && h[0] == 1 && h[1] == 2 && (h[2] == 2 || h[2] == 3)) ? 2 : 3;
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] v_cvt_pk_u8_f32(0.7, 1.5, 2.5, -3, 300) = %u %u %u %u %u -> mode %d\n", h[0], h[1], h[2], h[3], h[4], st);
    g_cvt_state.store(st, std::memory_order_release);
}
float cvt_bias(Ctx& c) {
    if (!c.dry && !c.grp) cvt_probe(c.st);         // (a group probes once, on the calling thread, before its members start)
    const int st = g_cvt_state.load(std::memory_order_acquire);
    return st == 1 ? 128.5f : st == 2 ? 128.0f : 0.0f;
}
// what k_pack1 covers: one int8 PACK_SYM plane in any layout, scales per plane / row block / batch block -- a single plane, or
// the one candidate of a device-side range that the host knows to hold at most one
inline bool pack1_ok(const PackParams& p, int live_max) {
    return p.mode == PACK_SYM && !p.conv && !(p.blk_mode == 1 && p.blk_div2) && p.lo >= -128 && p.hi <= 127 && p.lo <= p.hi &&
           (p.crange ? live_max == 1 : p.C == 1) && (p.c_inner != 3 || (p.Rp % 64 == 0 && p.Kp % 64 == 0));
}
std::atomic<int> g_pack_general{0};   // p4v_debug_pack_cands: single planes through k_pack as well (kernel-vs-kernel test)
// `live_max`: what the host knows of a pruned launch -- an upper bound of the number of candidates in p.crange - p.c_base that
// fall inside [0, p.C) (< 0: nothing; 0: none, no launch).  The candidate groups of k_pack are counted from the first candidate
// of the range, so ceil(live_max / PACK_CG) of them cover it wherever it lies.
template <typename T> int launch_pack(Ctx& c, const PackParams& p_, int live_max = -1) {
    if (c.dry) return 0;
    PackParams p = p_;
    if (p.crange && live_max == 0) return 0;
    // the full symmetric 8-bit grid: quant16_sat8 once the conversion has been probed (the *_impl entry points do that first);
    // tuning 12 = 11 keeps quant_fast1 (A/B)
    p.qbias = (sizeof(T) == 1 && p.mode == PACK_SYM && p.lo == -128 && p.hi == 127 && tune(TUNE_B1_PATH) != 11) ? cvt_bias(c) : 0.0f;
    const long total = (long)p.Z * p.Rp * (p.Kp / 16);
    if (total >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "operand plane too large for k_pack (%ld 16-element runs)", total);
    // candidate groups: all of C, or -- a pruned launch whose length the host knows -- the ones that can be live
    const int groups = cdiv((p.crange && live_max > 0) ? std::min(p.C, live_max) : p.C, PACK_CG);
    // A pruned launch of unknown length lets most of its groups exit at once: fewer, longer-running workgroups.  One whose
    // groups are all live is an unpruned launch of that many groups: the same 256 * 64 workgroups over all of them.
    const long cap = !p.crange ? 256L * 64 : live_max > 0 ? std::max(256L * 12, 256L * 64 / groups) : 256L * 12;
    const int blocks = (int)std::min<long>(cdiv(total, 256), cap);
    if (p.mode == PACK_TWIN_I8) {
        if (sizeof(T) != 1 || p.C != 1 || p.c_inner != 0 || !p.scales || p.conv || p.zdiv > 0)
            return fail(P4V_ERR_UNSUPPORTED, "merged twin plane: one fixed row-major int8 plane only");
        return enqueue(c, KERN(PackParams, k_pack_twin), dim3(blocks), dim3(256), 0, p);
    }
    const bool single = sizeof(T) == 1 && pack1_ok(p, live_max) && !g_pack_general.load(std::memory_order_relaxed);
    if (tune(TUNE_PRINT) > 1) fprintf(stderr, "[p4v] %s stage %d: Z %d Rp %d Kp %d C %d crange %d done %d live_max %d layout %d grid %d x %d\n", single ? "k_pack1" : "k_pack", g_stage, p.Z, p.Rp, p.Kp, p.C, p.crange != nullptr, p.done != nullptr, live_max, p.c_inner, blocks, single ? 1 : groups);
    if (single) return enqueue(c, KERN(PackParams, k_pack1), dim3(blocks), dim3(256), 0, p);
    return enqueue(c, KERN_T(PackParams, k_pack, T), dim3(blocks, groups), dim3(256), 0, p);
}

// (inside a group the lock-step members share the chip: each plans for its share of the workgroup slots)
// `kind`: the sweep family (StatInfo.kind) -- what the group's last launch of that family held is the better estimate of how many
// members are in lock step than the number of same-shaped members
inline int lockstep(const Ctx& c, int kind) {
    if (!c.grp) return 1;
    const int seen = (kind >= 0 && kind < 16) ? c.grp->last_par[kind] : 0;
    return std::max(1, seen > 0 ? seen : c.par);
}
inline int cu_slots(const Ctx& c, int slots, int kind) { return std::max(8, slots / lockstep(c, kind)); }
// epilogue dispatch of a kernel family: E = the metric's epilogue as a template argument
#define P4V_EPI4(epi, X)                                   \
    switch (epi) {                                         \
        case EPI_SQ_W: { constexpr int E = EPI_SQ_W; X; }  \
        case EPI_SQ: { constexpr int E = EPI_SQ; X; }      \
        case EPI_ABS: { constexpr int E = EPI_ABS; X; }    \
        default: { constexpr int E = EPI_W_SQ; X; }        \
    }

template <typename T, bool TWIN> int launch_sweep_epi(Ctx& c, const SweepParams& p, int epi, int cgroups, const StatInfo* si) {
    const size_t lds = 2 * (TWIN ? 3 : 2) * SW_TILE_BYTES;
    dim3 grid(p.mtiles * p.ntiles, p.Z, cgroups), block(512);
    switch (epi) {
        case EPI_SQ_W: return enqueue(c, KERN_T(SweepParams, k_sweep, T, TWIN, EPI_SQ_W), grid, block, lds, p, si);
        case EPI_SQ: return enqueue(c, KERN_T(SweepParams, k_sweep, T, TWIN, EPI_SQ), grid, block, lds, p, si);
        case EPI_ABS: return enqueue(c, KERN_T(SweepParams, k_sweep, T, TWIN, EPI_ABS), grid, block, lds, p, si);
        case EPI_W_SQ: return enqueue(c, KERN_T(SweepParams, k_sweep, T, TWIN, EPI_W_SQ), grid, block, lds, p, si);
        case EPI_STORE: return enqueue(c, KERN1_T(SweepParams, k_sweep, T, TWIN, EPI_STORE), grid, block, lds, p, si);
        case EPI_FWD: return enqueue(c, KERN1_T(SweepParams, k_sweep, T, TWIN, EPI_FWD), grid, block, lds, p, si);
        default: return enqueue(c, KERN1_T(SweepParams, k_sweep, T, TWIN, EPI_COS), grid, block, lds, p, si);
    }
}

// k_sweep2g: large K, column operand expanded, row operand invariant (weight search): two candidates per pass
template <bool TWIN> int launch_sweep2g_epi(Ctx& c, const SweepParams& p, int epi, int cgroups, const StatInfo* si) {
    const int per = 2 * cdiv(p.c1 - p.c0, 2 * cgroups);
    const size_t lds = (size_t)SW2_NS * (TWIN ? 4 : 3) * SW2_TILE + (size_t)per * 8 * sizeof(float) * (TWIN ? 3 : 2);
    dim3 grid(p.mtiles * p.ntiles, p.Z, cgroups), block(512);
    P4V_EPI4(epi, return enqueue(c, KERN_T(SweepParams, k_sweep2g, TWIN, E), grid, block, lds, p, si))
}

template <bool TWIN> int launch_sweep2_epi(Ctx& c, const SweepParams& p, int epi, int cgroups, const StatInfo* si) {
    const int per = cdiv(p.c1 - p.c0, cgroups);
    const size_t lds = (size_t)SW2_NS * (TWIN ? 3 : 2) * SW2_TILE + (size_t)per * 8 * sizeof(float) * (TWIN ? 3 : 2);
    dim3 grid(p.mtiles * p.ntiles, p.Z, cgroups), block(512);
    switch (epi) {
        case EPI_SQ_W: return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_SQ_W), grid, block, lds, p, si);
        case EPI_SQ: return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_SQ), grid, block, lds, p, si);
        case EPI_ABS: return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_ABS), grid, block, lds, p, si);
        case EPI_FWD: return enqueue(c, KERN1_T(SweepParams, k_sweep2, TWIN, EPI_FWD), grid, block, lds, p, si);
        case EPI_STORE:     // (the twin instance has no register to spare for the group prologue: single launches)
            if constexpr (TWIN) return enqueue(c, KERN1_T(SweepParams, k_sweep2, TWIN, EPI_STORE), grid, block, lds, p, si);
            else return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_STORE), grid, block, lds, p, si);
        case EPI_COS: return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_COS), grid, block, lds, p, si);
        default: return enqueue(c, KERN_T(SweepParams, k_sweep2, TWIN, EPI_W_SQ), grid, block, lds, p, si);
    }
}

#ifdef P4V_TRACE
// tuning builds only (-DP4V_TRACE): per-workgroup timestamps of the stationary sweeps, appended to $P4V_TRACE_FILE
unsigned long long* g_trace = nullptr;
int trace_attach(Sweep3Params& p) {
    if (!g_trace) HIPCHK(hipMalloc(&g_trace, sizeof(unsigned long long) * 16 * 65536));
    p.trace = g_trace;
    return 0;
}
int trace_dump(Ctx& c, dim3 grid, int ktiles) {
    if (!getenv("P4V_TRACE_FILE")) return 0;
    const size_t n = (size_t)grid.x * grid.z * 16;
    HIPCHK(hipStreamSynchronize(c.st));
    std::vector<unsigned long long> h(n);
    HIPCHK(hipMemcpy(h.data(), g_trace, n * 8, hipMemcpyDeviceToHost));
    FILE* f = fopen(getenv("P4V_TRACE_FILE"), "ab");
    unsigned long long hdr[4] = {0xABCDull, grid.x, grid.z, (unsigned long long)ktiles};
    fwrite(hdr, 8, 4, f); fwrite(h.data(), 8, n, f); fclose(f);
    return 0;
}
#endif

// the record of a timed sweep launch (bench.py roofline): every launch is recorded, also a stage whose device-side candidate
// range is empty -- the records are the production launches, 1:1 with a kernel trace
inline StatInfo stat_info(int kind, double macs, double alg, int gx, int gz, double bytes) {
    return StatInfo{kind, macs * g_exec_frac, alg * g_exec_frac, g_stage, gx, gz, bytes};
}

// The sweep kernel family of a pass, decided once by plan_sweep ("pass -> kernel": the same order), and the
// family number of its launch records (p4v_launch_record.kind)
enum SweepKind { SK_BOUND, SK_SWEEP6, SK_SWEEP5, SK_SWEEP7, SK_SWEEP7_TWIN, SK_SWEEP7_MERGED, SK_SWEEP9, SK_SWEEP8, SK_SWEEP2G, SK_SWEEP2,
                 SK_GENERIC_I8, SK_GENERIC_F32, SK_COUNT };
constexpr int SWEEP_RECORD_KIND[SK_COUNT] = {12, 2, 5, 3, 4, 4, 6, 7, 8, 9, 0, 1};
inline bool sweep_stationary(SweepKind k) { return k == SK_SWEEP6 || k == SK_SWEEP5; }
inline bool sweep_large_k(SweepKind k) { return k == SK_SWEEP7 || k == SK_SWEEP7_TWIN || k == SK_SWEEP7_MERGED; }

int launch_sweep5(Ctx& c, const Sweep3Params& p, int epi, int cgroups) {
    if (c.dry) return 0;
    const int per = 2 * cdiv(p.c1 - p.c0, 2 * cgroups);
    const size_t lds = (size_t)p.ktiles * SW2_TILE + (size_t)SW5_NP * 2 * SW2_TILE + (size_t)per * 8 * sizeof(float) * 2 + 256;
    dim3 grid(p.stiles * p.ttiles, 1, cgroups), block(512);
#ifdef P4V_TRACE
    CHK(trace_attach(const_cast<Sweep3Params&>(p)));
#endif
    const StatInfo si = stat_info(SWEEP_RECORD_KIND[SK_SWEEP5], (double)p.stiles * 128 * (double)p.ttiles * 128 * (double)p.ldk * (p.c1 - p.c0), g_alg_macs_cand * (p.c1 - p.c0),
                                  (int)grid.x, (int)grid.z, g_alg_bytes);
    const StatInfo* sp = &si;
    P4V_EPI4(epi, CHK(enqueue(c, KERN_T(Sweep3Params, k_sweep5, E), grid, block, lds, p, sp)); break)
#ifdef P4V_TRACE
    CHK(trace_dump(c, grid, p.ktiles));
#endif
    return 0;
}

template <int KT>
int launch_sweep6_kt(Ctx& c, const Sweep3Params& p, int epi, dim3 grid, size_t lds, const StatInfo* si) {
    // (cosine: plain = activation search, transposed = weight search)
    if (epi == EPI_COS) return enqueue(c, KERN_T(Sweep3Params, k_sweep6, EPI_COS, KT, 2), grid, dim3(256), lds, p, si);
    if (epi == EPI_COS_T) return enqueue(c, KERN_T(Sweep3Params, k_sweep6, EPI_COS_T, KT, 2), grid, dim3(256), lds, p, si);
    P4V_EPI4(epi, return enqueue(c, KERN_T(Sweep3Params, k_sweep6, E, KT, 2), grid, dim3(256), lds, p, si))
}

// k_sweep6 (stationary operand in registers): K = 192 / 256 / 384 / 512 / 768 bytes -- the Linear layers of
// ViT/DeiT-T/S/B and of Swin stages 2-3
bool sweep6_supported(int ktiles) { return ktiles == 3 || ktiles == 4 || ktiles == 6 || ktiles == 8 || ktiles == 12; }

int launch_sweep6_part(Ctx& c, const Sweep3Params& p, int epi, int cgroups);

// One workgroup per CU (512 registers per wave): `tiles` equal workgroups run in ceil(tiles / 256) waves and the last
// one is mostly empty (ViT-B qkv: 900 tiles = 3.5 waves).  The tiles of the last, partial wave are launched separately
// with their candidates split over q groups, so that it takes a fraction of a full wave's time; every group pays
// the workgroup prologue (stationary operand + raw_out / raw_grad tile) again.  Cost model in microseconds.
// (Inside a group the other members' tiles fill the last wave: no split.)
int launch_sweep6(Ctx& c, const Sweep3Params& p, int epi, int cgroups, int nc_model = 0) {
    if (c.dry) return 0;
    // (p.ntile > 0: only the tiles [p.tile0, p.tile0 + p.ntile) -- the open score blocks of a pruned pass; nc_model: the number of
    // candidates the device-side range leaves, when the host knows it)
    const int tiles = p.ntile > 0 ? p.ntile : p.stiles * p.ttiles, base = p.ntile > 0 ? p.tile0 : 0;
    const int nc = nc_model > 0 ? nc_model : p.c1 - p.c0;
    const int full = tiles / 256 * 256, rem = tiles - full;
    const double P = tune(TUNE_P6) > 0 ? 0.1 * tune(TUNE_P6) : 20.0, t_c = 0.196 * p.ktiles;        // prologue, one candidate of one tile
    auto waves = [](long wgs) { return (double)((wgs + 255) / 256); };
    int q_best = 0;
    if (rem > 0 && full > 0 && lockstep(c, 2) <= 1) {
        double best = waves((long)tiles * cgroups) * (P + cdiv(nc, cgroups) * t_c) * 0.97;   // the uniform plan
        for (int q = 1; q <= std::min(nc, 12); ++q) {
            const double t = waves(full) * (P + nc * t_c) + waves((long)rem * q) * (P + cdiv(nc, q) * t_c);
            if (t < best) { best = t; q_best = q; }
        }
    }
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] sweep6 tiles %d: full %d rem %d -> q %d (uniform cg %d)\n", tiles, full, rem, q_best, cgroups);
    if (q_best > 0) {
        Sweep3Params a = p, b = p;
        a.tile0 = base; a.ntile = full;
        b.tile0 = base + full; b.ntile = rem;
        CHK(launch_sweep6_part(c, a, epi, 1));
        CHK(launch_sweep6_part(c, b, epi, q_best));
    } else {
        Sweep3Params a = p;
        a.tile0 = base; a.ntile = p.ntile > 0 ? tiles : 0;
        CHK(launch_sweep6_part(c, a, epi, cgroups));
    }
    return 0;
}

int launch_sweep6_part(Ctx& c, const Sweep3Params& p, int epi, int cgroups) {
    const int per = cdiv(p.c1 - p.c0, cgroups);
    const int nw = 4;       // waves per workgroup, one per SIMD
    const size_t lds = (size_t)3 * p.ktiles * 4096 + (size_t)(per + 1) * 2 * nw * sizeof(float) + (size_t)per * nw * sizeof(float) + 64 * sizeof(float) + 256;
    dim3 grid(p.ntile > 0 ? p.ntile : p.stiles * p.ttiles, 1, cgroups);
#ifdef P4V_TRACE
    CHK(trace_attach(const_cast<Sweep3Params&>(p)));
#endif
    // one record per kernel launch; a split sweep books its work (and the pass's bytes) in proportion to the tiles of each part
    const double share = (double)grid.x / ((double)p.stiles * p.ttiles);
    const StatInfo si = stat_info(SWEEP_RECORD_KIND[SK_SWEEP6], share * (double)p.stiles * 256 * (double)p.ttiles * 64 * (double)p.ldk * (p.c1 - p.c0),
                                  share * g_alg_macs_cand * (p.c1 - p.c0), (int)grid.x, (int)grid.z, share * g_alg_bytes);
    const StatInfo* sp = &si;
    int r;
    switch (p.ktiles) {
        case 12: r = launch_sweep6_kt<12>(c, p, epi, grid, lds, sp); break;
        case 8: r = launch_sweep6_kt<8>(c, p, epi, grid, lds, sp); break;
        case 6: r = launch_sweep6_kt<6>(c, p, epi, grid, lds, sp); break;
        case 4: r = launch_sweep6_kt<4>(c, p, epi, grid, lds, sp); break;
        default: r = launch_sweep6_kt<3>(c, p, epi, grid, lds, sp); break;
    }
    if (r) return r;
#ifdef P4V_TRACE
    CHK(trace_dump(c, grid, p.ktiles));
#endif
    return 0;
}

// k_sweep9: single-k-tile sweeps on 16 x 16 blocks (part layout [C][Z][halves * 8], set up by plan_sweep)
template <bool ROWS_FIXED> int launch_sweep9_epi(Ctx& c, const SweepParams& p, int epi, int cgroups, const StatInfo* si) {
    const int per = cdiv(p.c1 - p.c0, cgroups);
    const size_t lds = (size_t)SW9_NS * SW9_STAGE + (size_t)per * SW9_NW * sizeof(float) * 2;
    dim3 grid(p.halves, p.Z, cgroups), block(SW9_NW * 64);
    P4V_EPI4(epi, return enqueue(c, KERN_T(SweepParams, k_sweep9, ROWS_FIXED, E), grid, block, lds, p, si))
}

// k_sweep8: single k-tile (K <= 64) int8 sweep with the fixed operand's fragments in registers: q.k^T of every ViT / Swin
// (no padding skip as in k_sweep2 -- wave parts without a valid element doing no MFMA / epilogue work: measured slower at 197
// tokens, 4 of 32 parts padding: 459 vs 428 us, AND at the 144 tokens of a Swin window, 17 of 32 parts: 10.0 vs 9.3 ms per
// module -- a single-k-tile candidate is paced by its ring step (DMA landing + barrier), not by the MFMAs and the epilogue it
// would skip.  k_sweep8's SKIP parameter is always false.)
template <bool ROWS_FIXED> int launch_sweep8_epi(Ctx& c, const SweepParams& p, int epi, int cgroups, const StatInfo* si) {
    const int per = cdiv(p.c1 - p.c0, cgroups);
    const size_t lds = (size_t)SW8_NS * SW2_TILE + (size_t)per * 8 * sizeof(float) * 2;
    dim3 grid(p.mtiles * p.ntiles, p.Z, cgroups), block(512);
    P4V_EPI4(epi, return enqueue(c, KERN_T(SweepParams, k_sweep8, ROWS_FIXED, E, false), grid, block, lds, p, si))
}

// k_sweep7: large-K int8 sweep (both operands streaming, 256 x 256 workgroup tile)
template <int TWIN> int launch_sweep7_epi(Ctx& c, const Sweep7Params& p, int epi, dim3 grid, size_t lds, const StatInfo* si) {
    if constexpr (TWIN == 0) { if (epi == EPI_COS) return enqueue(c, KERN_T(Sweep7Params, k_sweep7, 0, EPI_COS), grid, dim3(512), lds, p, si); }
    if (epi == EPI_COS) return fail(P4V_ERR_UNSUPPORTED, "k_sweep7: the cosine epilogue has no twin instance");
    P4V_EPI4(epi, return enqueue(c, KERN_T(Sweep7Params, k_sweep7, TWIN, E), grid, dim3(512), lds, p, si))
}

int launch_sweep7(Ctx& c, const Sweep7Params& p, int twin, int epi, int cgroups) {   // twin: 0 plain, 1 two planes, 2 merged plane
    if (c.dry) return 0;
    const int nc = p.c1 - p.c0;
    // the per-candidate tables live behind the ring: at most 160 candidates per workgroup
    const int per_max = (int)((160 * 1024 - SW7_NS * SW7_STAGE - 256) / 192);
    cgroups = std::max(cgroups, cdiv(nc, per_max));
    const int per = cdiv(nc, cgroups);
    const size_t lds = (size_t)SW7_NS * SW7_STAGE + (size_t)per * 192 + 256;
    Sweep7Params q = p;
    q.cgroups = cgroups;
    dim3 grid(p.rtiles * p.ctiles * cgroups, 1, 1);
    // (twin: 128 samples x 2 planes)
    const StatInfo si = stat_info(SWEEP_RECORD_KIND[twin ? SK_SWEEP7_TWIN : SK_SWEEP7], (double)p.rtiles * 256 * (double)p.ctiles * 256 * (double)p.ldk * nc, g_alg_macs_cand * nc,
                                  (int)grid.x, (int)grid.z, g_alg_bytes);
    const StatInfo* sp = &si;
    return twin == 2 ? launch_sweep7_epi<2>(c, q, epi, grid, lds, sp) : twin ? launch_sweep7_epi<1>(c, q, epi, grid, lds, sp) : launch_sweep7_epi<0>(c, q, epi, grid, lds, sp);
}

// the tiled sweeps (one SweepParams): the launch of `kind` and its record, whose grid_x is the arm's own grid
int launch_sweep(Ctx& c, const SweepParams& p, SweepKind kind, bool twin, int epi, int cgroups) {
    if (c.dry) return 0;
    const double kelems = (double)p.ldk / (kind == SK_GENERIC_F32 ? 4 : 1);
    const int tiles = p.mtiles * p.ntiles;
    auto record = [&](int gx) {
        return stat_info(SWEEP_RECORD_KIND[kind], (double)p.mtiles * SW_BM * (double)p.ntiles * SW_BN * kelems * p.Z * (p.c1 - p.c0) * (twin ? 2 : 1),
                         g_alg_macs_cand * (p.c1 - p.c0), gx, cgroups, g_alg_bytes);
    };
    switch (kind) {
        case SK_BOUND: {
            // 128 x 128 workgroup tiles, 64 x 64 per wave; the comparison path (tuning 12 = 4): 128 x 64 tiles, 64 x 32 per wave
            const bool prev = b1_previous();
            const StatInfo si = record(tiles * (prev ? 2 : 1));
            const dim3 grid(tiles * (prev ? 2 : 1)), block(256);
            if (prev) P4V_EPI4(epi, return enqueue(c, KERN_T(SweepParams, k_bound, E, 1), grid, block, 0, p, &si))
            P4V_EPI4(epi, return enqueue(c, KERN_T(SweepParams, k_bound, E, 2), grid, block, 0, p, &si))
        }
        case SK_SWEEP9: {
            const StatInfo si = record(p.halves);
            return p.a_cs == 0 ? launch_sweep9_epi<true>(c, p, epi, cgroups, &si) : launch_sweep9_epi<false>(c, p, epi, cgroups, &si);
        }
        case SK_SWEEP8: {
            const StatInfo si = record(tiles);
            return p.a_cs == 0 ? launch_sweep8_epi<true>(c, p, epi, cgroups, &si) : launch_sweep8_epi<false>(c, p, epi, cgroups, &si);
        }
        case SK_SWEEP2G: {
            const StatInfo si = record(tiles);
            return twin ? launch_sweep2g_epi<true>(c, p, epi, cgroups, &si) : launch_sweep2g_epi<false>(c, p, epi, cgroups, &si);
        }
        case SK_SWEEP2: {
            const StatInfo si = record(tiles);
            return twin ? launch_sweep2_epi<true>(c, p, epi, cgroups, &si) : launch_sweep2_epi<false>(c, p, epi, cgroups, &si);
        }
        case SK_GENERIC_I8: {
            const StatInfo si = record(tiles);
            return twin ? launch_sweep_epi<int8_t, true>(c, p, epi, cgroups, &si) : launch_sweep_epi<int8_t, false>(c, p, epi, cgroups, &si);
        }
        case SK_GENERIC_F32: {
            const StatInfo si = record(tiles);
            return twin ? launch_sweep_epi<float, true>(c, p, epi, cgroups, &si) : launch_sweep_epi<float, false>(c, p, epi, cgroups, &si);
        }
        default: return fail(P4V_ERR_INVALID, "launch_sweep: family %d has a launcher of its own", (int)kind);
    }
}

int launch_finish(Ctx& c, const FinishParams& p) {
    return enqueue(c, KERN(FinishParams, k_finish), dim3(p.C, p.nj), dim3(256), 0, p);
}

int launch_finish_cos(Ctx& c, const FinishCosParams& p) {
    const int gy = p.j_mode == 3 ? cdiv(p.S, 256) : p.nj;
    return enqueue(c, KERN(FinishCosParams, k_finish_cos), dim3(p.C, gy), dim3(p.j_mode == 3 ? 256 : 1024), 0, p);
}

int launch_select(Ctx& c, const SelectParams& p_) {
    if (c.dry) return 0;
    SelectParams p = p_;
    attach_mirror(p);
    return enqueue(c, KERN(SelectParams, k_select), dim3(p.nj), dim3(128), 0, p);
}

// ---- one search pass -------------------------------------------------------------------------------
// A "pass" evaluates eq_n candidates of ONE operand against a fixed counterpart and selects the best
// candidate per score block.  The GEMM is D[rows][cols] = rowop . colop^T; in the plain orientation rows
// are samples (activations / matmul A) and columns are output features (weights / matmul B); the cosine
// metric runs swapped so that the feature axis it reduces over lies on the MFMA rows.
// The candidate-expanded plane of one search (weights x 100 scales, ...) depends on the operand and on the candidate
// table only -- both fixed for the whole calibration_step2 (the table is built once from the INITIAL interval,
// reference linear.py:544-545) -- so rounds 2..R find it already packed.  One object per (module, searched operand),
// owned by the *_impl call; the buffer lives at the top of the workspace.
struct PlaneCache {
    char* buf = nullptr;
    bool assigned = false, valid = false;
    unsigned char* done = nullptr;    // pruned passes: device flags, one per candidate already in `buf`
};
// The sample slice of the pruned passes (run_pass_pruned, stage A): which samples carry the metric weight depends on raw_grad /
// raw_out only, so the ranking, the gathered rows of raw_out / raw_grad and of the row operand are built by the first pruned pass
// of a module and reused by the others (both searches, all rounds); a buffer is gathered again only when its source changed
// (the folded target of the twin activation search is rebuilt per pass).
struct SliceCache {
    bool assigned = false;
    int k = 0;                        // rows per segment the buffers are sized for
    int k_eff = 0;                    // rows per segment in use (a Linear whose 256 heaviest samples hold the weight uses those)
    int* idx = nullptr; float* mass = nullptr;
    float* Os = nullptr; float* Gs = nullptr; float* Rs = nullptr;
    const void* idx_src = nullptr; int idx_wt = -1;      // what the ranking was computed from
    const void* o_src = nullptr; const void* g_src = nullptr; const void* r_src = nullptr;
    float* frac = nullptr;            // device: share of the metric weight the slice holds
    PlaneCache aplane;                // stage A's candidate-expanded plane of the SLICED operand (the search whose row operand is
                                      // expanded): candidates and slice rows are fixed for the call, the later rounds find it packed
    bool loose = false;               // that share is too small for the stages to pay (Swin: no class token): full sweeps
    float frac_host = 1.0f;           // that share as the host read it (0 < f < 1 once measured): decides about the second tier
};
// The same for the epilogue operands of k_sweep6 in fragment order (k_prep_epi6): raw_out, raw_grad and the bias are fixed
// for the whole call, so the tile image of one search orientation is built by its first pass and read by the later rounds.
typedef PlaneCache EpiCache;

struct Operand {
    PackParams pk;        // src/strides/sizes/scales/mode filled by the caller (dst, C, Rp, Kp set by run_pass)
    bool expanded;        // true: one plane per candidate
    bool present;
    bool prepacked;       // a forward pass only: `plane` is the operand's fixed int8 plane, row-major [pl.Mp][pl.Kp] (row / row2) or
    const void* plane;    // [pl.NpB][pl.Kp] (col) as plan_sweep sizes it, written by an earlier launch on the stream (mlp_impl: fc1's
                          // epilogue; qkv_attn_impl: k_qkv_heads); nothing is allocated or packed for it (a sizing run: no address
                          // yet).  false (everything else): packed from pk.src
};

// A MatMul pass with row / column sub-blocks (n_V, n_H > 1; matmul_impl): the K axis cut where either operand's scale changes
// (p4v_kernels.h, "MatMul sub-block scales"), both interval tensors, and -- for a search step -- the ONE block whose candidates
// are swept (reference matmul.py:489-521 / 530-562: every other block keeps the interval entering the step).
struct SegPlan {
    SegTable seg; unsigned char ablk[SEG_MAX], bblk[SEG_MAX]; int Kseg;
    int batch, H, M, K, N;
    int nVA, nHA, nVB, nHB, crA, ccA, crB, ccB;     // block counts; rows / columns per block (ceil, matmul.py:109-122)
    const float* A; long a_st[4]; const float* B; long b_st[4];
    int Aq, Bq; bool sos;
    const float* ivA; const float* ivB;             // [H][nVA][nHA] / [H][nVB][nHB]; sos: ivA = the scalar A_interval
    const float* split;                             // sos
    int side, ov_v, ov_h;                           // 0: forward; 1 / 2: the searched block of A / B
    const float* cands; int cand_cs, cand_hs;       // its candidates: cands[c * cand_cs + head * cand_hs]
    bool b_shared;                                  // B and its intervals [nVB][nHB] are the same for every head (b_st[0] = b_st[1] = 0):
                                                    // ONE plane of B -- the activations of a Linear layer (linear_impl)
};

struct Pass {
    bool i8, twin;
    int epi, wt_mode;
    Operand row, row2, col;   // row2 = twin second plane (always on the row side)
    int Z;                    // batched GEMMs (matmul batch*heads, V blocks of the swapped cosine sweep)
    long row_zs_shared, col_zs_shared;  // 1 = operand shared across z (stride 0)
    int Mrows, Ncols, K;      // valid sizes of the GEMM
    int eq_n;
    // scales
    ScaleParams s1, s2;       // s.S filled by run_pass; nblk = s_cs
    bool use_s1;
    int sb_mode, sb_div, s_cs;
    // epilogue operands
    const float* bias; int bias_axis; long bias_zs;
    const float* O; const float* G;
    long o_zs, o_bs, o_ms, o_nbs, o_ns; int o_inner, o_ninner;
    // finish
    int j_mode, j_div, nj; double norm;
    int cos_ZB, cos_ZV, cos_j_mode, cos_j_div;   // cosine finish geometry
    // select
    const float* cands; int cand_cs, cand_js, cand_off;
    float* interval; int out_js, out_off;
    float* aux_out; float aux_div;
    float* scores_out; int scores_out_ld;
    int32_t* best_out;
    float* store_out;         // where a storing pass writes (the address only: null in a sizing run)
    // EPI_STORE (raw_out - bias - scale*acc) / EPI_FWD (the quantised product): one "candidate", stored, no finish / select
    bool stores() const { return epi == EPI_STORE || epi == EPI_FWD; }
    bool cos6;                // cosine of a plain Linear layer on k_sweep6 (rows = samples, cols = features, Z = 1): set by linear_impl
    bool cos7;                // ... on k_sweep7 (K >= 1024)
    bool twin_disjoint;       // twin whose two ranges never overlap (post-GELU): k_sweep7 may stream them as one merged plane
    // exact candidate pruning (run_pass_pruned): device-side candidate range, scores kept for the next stage, no selection
    const int* crange;
    const int* crange_blk;    // ... and per score block [2 * nj] (k_prune_hull's rblk): honoured where the sweep kernel's tiles lie inside
                              // one score block (run_pass decides; otherwise every block sweeps `crange`, a superset)
    int host_lo, host_hi;     // what the host read of `crange` (host_hi > host_lo: known) -- the launch geometry is planned for the
    const int* host_rblk;     // candidates that will run -- and of `crange_blk` (nj <= MIR_BLK; nullptr: unknown): closed blocks are not launched
    int host_len;             // > 0: the host does not know where `crange` lies but knows it holds at most this many candidates
                              // (stage B1 of a single score block: the slice winner) -- k_pack launches that many, counted from crange[0]
    float* scores_keep;
    bool no_select;
    bool prunable;            // set by the *_impl callers for passes whose score is minus a sum of non-negative terms
    bool prunable_f32;        // ... and which may be pruned although their operands are fp32 planes (conv with a_bit >= 32)
    float* S1_pre; float* S2_pre; bool s_ready;   // scale tables shared by the stages of a pruned pass (same table, same scales)
    SliceCache* scache;       // optional: the module's sample slice, shared by its pruned passes
    SliceCache* scache2;      // optional (Linear): the module's second, larger slice (two-tier pruning, run_pass_pruned)
    bool bound_kernel;        // stage B1 of a pruned pass: ONE candidate over all samples -> k_bound where the layout allows it
    bool host_sync_ok;        // the caller synchronises the stream after the pass anyway (pass memo): the pruned pass may read
                              // the 8-byte survivor range back and skip the launches of an empty stage B2
    PlaneCache* cache;        // optional: keeps the candidate-expanded plane across the rounds of one call
    EpiCache* ecache;         // optional: keeps k_sweep6's fragment-order epilogue operands across the rounds of one call
    bool pack_only;           // plan the pass and pack its candidate-expanded operand into `cache`, nothing else (linear_impl: the
                              // candidate planes of the WEIGHTS depend on no captured tensor -- packed while the capture still runs)
    const SegPlan* seg;       // MatMul sub-block scales: the K-segment table and the two block-scale tables -> k_pack_seg / k_sweep_seg
                              // (run_pass_seg); the operands, scales and candidates of such a pass are described there
};

static const long PLANE_BUDGET_DEFAULT = 6L << 30;  // bytes of candidate-expanded plane kept resident per chunk
#define PLANE_BUDGET (tune(TUNE_PLANE_GIB) > 0 ? ((long)tune(TUNE_PLANE_GIB) << 30) : PLANE_BUDGET_DEFAULT)
#define PLANE_CACHE_MAX (PLANE_BUDGET / 2)      // largest candidate-expanded plane kept across the rounds of one call

// How many candidate groups (gridDim.z) to split a sweep into.  Splitting raises the workgroup count (fills the
// 256 CUs / evens out the last round) but every workgroup pays its prologue (raw_out/raw_grad tile, stationary
// operand) again.  Cost model in microseconds, constants measured on MI355X (profiles/): minimise
// rounds * (prologue + candidates_per_group * ktiles * tile_time).
int choose_cgroups(long wgs, int ncand, int ktiles, int slots, double prologue_us, double tile_us, int cg_max = 25) {
    int best = 1;
    double best_t = 1e30;
    for (int cg = 1; cg <= std::min(ncand, cg_max); ++cg) {
        const long rounds = (wgs * cg + slots - 1) / slots;
        const double t = (double)rounds * (prologue_us + (double)cdiv(ncand, cg) * ktiles * tile_us);
        if (t < best_t * 0.999) { best_t = t; best = cg; }
    }
    return best;
}

// the two fixed planes of a twin row operand can come from one launch: same source view, one scale each, plain modes
bool dual_pack_ok(const PackParams& a, const PackParams& b) {
    auto plain = [](const PackParams& p) {
        return (p.mode == PACK_SYM || p.mode == PACK_SOS_HI || p.mode == PACK_SOS_LO) && p.blk_mode == 0 && !p.conv && !p.crange;
    };
    return plain(a) && plain(b) && a.src == b.src && a.R == b.R && a.K == b.K && a.s_r == b.s_r && a.s_k == b.s_k &&
           a.s_z == b.s_z && a.s_z2 == b.s_z2 && a.zdiv == b.zdiv;
}

int launch_pass_select(Ctx& c, const Pass& ps, const float* scores) {
    SelectParams sl{scores, ps.eq_n, ps.nj, ps.cands, ps.cand_cs, ps.cand_js, ps.cand_off, ps.interval, ps.out_js,
                    ps.out_off, ps.aux_out, ps.aux_div, ps.scores_out, ps.scores_out_ld, ps.best_out};
    return launch_select(c, sl);
}

// ---- the sub-block pass (MatMul; cosine Linear with column / activation blocks): k_pack_seg planes, k_sweep_seg, then the
// common finish (k_finish; EPI_COS: k_finish_cos) and selection -----------------------------------------------------------------
int launch_pack_seg(Ctx& c, PackSegParams p) {
    if (c.dry) return 0;
    p.qbias = (p.mode == PACK_SYM && p.lo == -128 && p.hi == 127) ? cvt_bias(c) : 0.0f;
    const long total = (long)p.Z * p.Rp * (p.Kseg / 16);
    if (total >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "operand plane too large for k_pack_seg (%ld 16-element runs)", total);
    const int groups = cdiv(p.C, PACK_CG);
    return enqueue(c, KERN(PackSegParams, k_pack_seg), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 64), groups), dim3(256), 0, p);
}
template <bool TWIN> int launch_sweep_seg_epi(Ctx& c, const SweepSegParams& p, int epi, int cgroups, const StatInfo* si) {
    const size_t lds = 2 * (TWIN ? 3 : 2) * SW_TILE_BYTES + 2 * SEG_MAX * 128 * sizeof(float) + SEG_KT_MAX * sizeof(short) + 2 * SEG_MAX;
    dim3 grid(p.mtiles * p.ntiles, p.Z, cgroups), block(512);
    if (epi == EPI_FWD) return enqueue(c, KERN_T(SweepSegParams, k_sweep_seg, TWIN, EPI_FWD), grid, block, lds, p, si);
    if constexpr (!TWIN) { if (epi == EPI_COS) return enqueue(c, KERN_T(SweepSegParams, k_sweep_seg, false, EPI_COS), grid, block, lds, p, si); }
    if (epi == EPI_COS) return fail(P4V_ERR_UNSUPPORTED, "k_sweep_seg: the cosine epilogue has no twin instance");
    P4V_EPI4(epi, return enqueue(c, KERN_T(SweepSegParams, k_sweep_seg, TWIN, E), grid, block, lds, p, si))
}
int run_pass_seg(Ctx& c, Pass& ps) {
    const SegPlan& g = *ps.seg;
    const int Z = ps.Z, M = g.M, N = g.N, H = g.H, Kseg = g.Kseg;
    const bool fwd = ps.epi == EPI_FWD, cosm = ps.epi == EPI_COS;
    const int ZB = g.b_shared ? 1 : Z;                           // planes of B
    g_alg_macs_cand = (double)M * N * g.K * Z;
    g_alg_bytes = 4.0 * ((double)M * g.K * Z + (double)N * g.K * ZB) + (ps.G ? 8.0 : 4.0) * (double)M * N * Z;
    // (cosine: k_finish_cos's table, ceil(M / 64) slabs of (dot, |sim|^2, |raw|^2) per padded sample)
    const int Mp = (int)rup(M, SW_BM), Np = (int)rup(N, SW_BN), MT = cosm ? cdiv(M, 64) : Mp / 64;
    const long a_plane = (long)Z * Mp * Kseg, b_plane = (long)ZB * Np * Kseg;
    const bool a_exp = g.side == 1, b_exp = g.side == 2;
    const long exp_plane = a_exp ? a_plane : b_plane;
    const int chunk = (int)std::max<long>(1, std::min<long>(ps.eq_n, PLANE_BUDGET / std::max<long>(1, exp_plane)));
    const size_t mark = c.ws.off;
    char* abuf = c.ws.get<char>((size_t)a_plane * (a_exp ? chunk : 1));
    char* a2buf = g.sos ? c.ws.get<char>((size_t)a_plane) : nullptr;
    char* bbuf = c.ws.get<char>((size_t)b_plane * (b_exp ? chunk : 1));
    const long p_zs = (long)MT * Np * (cosm ? 3 : 1), p_cs = p_zs * Z;
    float* part = fwd ? nullptr : c.ws.get<float>((size_t)p_cs * ps.eq_n);
    float* scores = fwd ? nullptr : c.ws.get<float>((size_t)ps.eq_n * H);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    if (c.dry) { c.ws.off = mark; return 0; }

    auto a_pack = [&](int mode, char* dst, const float* cands, int C) {
        PackSegParams p{};
        p.src = g.A; p.s_z2 = g.a_st[0]; p.s_z = g.a_st[1]; p.s_r = g.a_st[2]; p.s_k = g.a_st[3]; p.zdiv = H;
        p.Z = Z; p.R = M; p.K = g.K; p.Rp = Mp; p.Kseg = Kseg; p.dst = dst; p.C = C;
        p.H = H; p.mode = mode; p.seg = g.seg;
        std::memcpy(p.kblk, g.ablk, sizeof p.kblk);
        if (mode == PACK_SYM) {
            p.iv = g.ivA; p.iv_hs = g.nVA * g.nHA; p.iv_rs = g.nHA; p.iv_ks = 1; p.r_div = g.crA; p.nblk_r = g.nVA;
            p.cands = cands; p.cand_cs = g.cand_cs; p.cand_hs = g.cand_hs; p.ov_r = g.ov_v; p.ov_k = g.ov_h;
            p.lo = -g.Aq; p.hi = g.Aq - 1;
        } else {                    // the split-of-softmax ranges: one scalar, the split (no blocks on A, matmul.py:586-588)
            p.iv = g.split; p.iv_hs = p.iv_rs = p.iv_ks = 0; p.r_div = std::max(1, M); p.nblk_r = 1;
            p.qm1 = (float)(g.Aq - 1);
        }
        return launch_pack_seg(c, p);
    };
    auto b_pack = [&](char* dst, const float* cands, int C) {
        PackSegParams p{};           // logical [Z][rows = n][K]: the row block is B's column block, the k block its row block
        p.src = g.B; p.s_z2 = g.b_st[0]; p.s_z = g.b_st[1]; p.s_r = g.b_st[3]; p.s_k = g.b_st[2]; p.zdiv = H;
        p.Z = ZB; p.R = N; p.K = g.K; p.Rp = Np; p.Kseg = Kseg; p.dst = dst; p.C = C;     // (b_shared: z = head = 0)
        p.H = H; p.mode = PACK_SYM; p.seg = g.seg;
        std::memcpy(p.kblk, g.bblk, sizeof p.kblk);
        p.iv = g.ivB; p.iv_hs = g.nVB * g.nHB; p.iv_rs = 1; p.iv_ks = g.nHB; p.r_div = g.ccB; p.nblk_r = g.nHB;
        p.cands = cands; p.cand_cs = g.cand_cs; p.cand_hs = g.cand_hs; p.ov_r = g.ov_h; p.ov_k = g.ov_v;
        p.lo = -g.Bq; p.hi = g.Bq - 1;
        return launch_pack_seg(c, p);
    };
    // fixed planes once
    if (g.sos) { CHK(a_pack(PACK_SOS_HI, abuf, nullptr, 1)); CHK(a_pack(PACK_SOS_LO, a2buf, nullptr, 1)); }
    else if (!a_exp) CHK(a_pack(PACK_SYM, abuf, nullptr, 1));
    if (!b_exp) CHK(b_pack(bbuf, nullptr, 1));
    for (int c0 = 0; c0 < ps.eq_n; c0 += chunk) {
        const int nc = std::min(chunk, ps.eq_n - c0);
        if (a_exp) CHK(a_pack(PACK_SYM, abuf, g.cands + (long)c0 * g.cand_cs, nc));
        if (b_exp) CHK(b_pack(bbuf, g.cands + (long)c0 * g.cand_cs, nc));
        SweepSegParams sp{};
        sp.a_cs = a_exp ? a_plane : 0; sp.A = abuf - (long)c0 * sp.a_cs; sp.a_zs = (long)Mp * Kseg;
        sp.A2 = a2buf; sp.a2_zs = sp.a_zs;
        sp.b_cs = b_exp ? b_plane : 0; sp.B = bbuf - (long)c0 * sp.b_cs; sp.b_zs = g.b_shared ? 0 : (long)Np * Kseg;
        sp.b_shared = g.b_shared; sp.bias = ps.bias; sp.bias_zs = ps.bias_zs;
        sp.ldk = Kseg; sp.ktiles = Kseg / SW_BKB;
        sp.ivA = g.sos ? nullptr : g.ivA; sp.ivB = g.ivB;
        sp.H = H; sp.nVA = g.nVA; sp.nHA = g.nHA; sp.nVB = g.nVB; sp.nHB = g.nHB; sp.m_div = g.crA; sp.n_div = g.ccB;
        sp.cands = g.cands; sp.cand_cs = g.cand_cs; sp.cand_hs = g.cand_hs; sp.side = g.side; sp.ov_v = g.ov_v; sp.ov_h = g.ov_h;
        sp.rs_const = 1.0f / (float)(g.Aq - 1); sp.rs2 = g.sos ? g.ivA : nullptr;
        sp.O = ps.O; sp.Wt = ps.G ? ps.G : ps.O; sp.wt_mode = ps.wt_mode; sp.o_zs = (long)M * N; sp.o_ms = N;
        sp.M = M; sp.N = N; sp.Z = Z; sp.c0 = c0; sp.c1 = c0 + nc; sp.crange = nullptr;
        sp.part = part; sp.p_cs = p_cs; sp.p_zs = p_zs; sp.Np = Np; sp.mtiles = Mp / SW_BM; sp.ntiles = Np / SW_BN;
        sp.store = ps.store_out;
        sp.seg = g.seg;
        std::memcpy(sp.ablk, g.ablk, sizeof sp.ablk); std::memcpy(sp.bblk, g.bblk, sizeof sp.bblk);
        // one workgroup per CU (512 threads, three or four register tiles per lane); per k-tile step as the generic int8 sweep
        const long wgs = (long)sp.mtiles * sp.ntiles * Z;
        const int cgroups = choose_cgroups(wgs, nc, sp.ktiles, cu_slots(c, 256, 15), 20.0, 1.6);
        const StatInfo si = stat_info(15, (double)Mp * Np * (double)Kseg * Z * nc * (g.sos ? 2 : 1), g_alg_macs_cand * nc,
                                      sp.mtiles * sp.ntiles, cgroups, g_alg_bytes);
        CHK(g.sos ? launch_sweep_seg_epi<true>(c, sp, ps.epi, cgroups, &si) : launch_sweep_seg_epi<false>(c, sp, ps.epi, cgroups, &si));
    }
    if (fwd) { c.ws.off = mark; return 0; }
    if (cosm) {
        FinishCosParams fp{part, p_cs, p_zs, Np, MT, ps.cos_ZB, ps.cos_ZV, N, ps.eq_n, ps.cos_j_mode, std::max(1, ps.cos_j_div), ps.nj, ps.norm, scores};
        CHK(launch_finish_cos(c, fp));
    } else {
        FinishParams fp{part, p_cs, p_zs, Np, MT, Z, N, ps.eq_n, ps.j_mode, std::max(1, ps.j_div), ps.nj, ps.norm, scores, nullptr};
        CHK(launch_finish(c, fp));
    }
    CHK(launch_pass_select(c, ps, scores));
    c.ws.off = mark;
    return 0;
}

// ---- the plan of a pass: which sweep kernel, and every size that follows from it ("pass -> kernel") -------------
struct SweepPlan {
    SweepKind kind;               // of a chunk of two or more candidates (chunk_kind)
    bool pairs;                   // k_sweep5: two candidates per pass, chunks start on a candidate pair
    bool merged7;                 // k_sweep7, post-GELU twin: ONE merged int8 plane k_pos + k_neg, split in registers
    bool b64;                     // k_sweep2, batched, N <= 64: the column operand's planes hold 64 rows
    bool fast_cos;                // cosine on k_sweep2 (three sums per sample and wave in k_sweep's table layout)
    bool epi6_on;                 // k_sweep6 reads its epilogue operands from the fragment-order image (k_prep_epi6)
    const int* rblk;              // Pass.crange_blk where the sweep honours it: k_sweep6's streaming tiles ...
    const int* rblk_z;            // ... / the z planes of the tiled sweeps (score block = z % heads)
    int esz, Kp, Mp, Np, NpB;     // operand element size; padded K / rows / columns; rows of the column operand's plane
    long row_plane1, col_plane1, exp_plane;      // bytes of one (candidate's) plane
    int chunk, chunk_al; size_t slack;           // candidates per chunk, padded to a pair; bytes the stationary rings read past the end
    int cin_exp, cin_fix;         // PackParams.c_inner of the expanded / the fixed operand
    size_t zero_bias_n, epi7_n;   // floats: the stationary sweeps' stand-in bias, k_sweep7's fragment-order epilogue operands
    int s6_stiles, s6_ttiles; size_t epi6_bytes; // k_sweep6: 256-row stationary slabs, 64-row streaming tiles, their epilogue image
    bool a_search;                // the row operand is expanded: stationary = weights (columns), streaming = activations
    long part_cs;                 // floats of partial-sum table per candidate (the allocation)
    long p_zs, p_cs; int NpP;     // the table the sweep writes: per z, per candidate, columns
    int s3_groups, cos6_Sp;       // its column count on the stationary sweeps / the padded samples of a cos6 / cos7 table
    int h9;                       // k_sweep9: halves per z
    long fin_zs; int fin_ld, fin_rows, fin_cols, fin_jdiv;   // k_finish / k_finish_cos: the same table as they read it
};

// k_sweep9: where the 128 x 128 tiles of k_sweep8 carry padding (>= 1.4 x the 16-granular area; DESIGN_LOG round 15 has the
// measurements).  Variant 1048576 forces it for A/B runs, 524288 disables it.  Returns the halves per z, 0: not this kernel.
int sweep9_halves(const Pass& ps, int ktiles) {
    const int epi = ps.epi;
    if (ktiles != 1 || ps.twin || ps.row.expanded == ps.col.expanded || epi == EPI_STORE || epi == EPI_FWD || epi == EPI_COS) return 0;
    if (ps.sb_mode == 1 && ps.s_cs > 1) return 0;
    if (ps.bias_axis != 0 || (g_variant & 524288)) return 0;
    // one ring stage holds the whole streamed operand of a candidate: 256 rows x 64 B (SW9_STAGE); beyond that k_sweep8
    if ((ps.row.expanded ? ps.Mrows : ps.Ncols) > 256) return 0;
    const long nb = (long)cdiv(ps.Mrows, 16) * cdiv(ps.Ncols, 16);
    const int halves = (int)cdiv(nb, (long)SW9_NW * SW9_NB);
    if (halves > 32 / SW9_NW) return 0;
    const double waste = (double)rup(ps.Mrows, 128) * rup(ps.Ncols, 128) / ((double)rup(ps.Mrows, 16) * rup(ps.Ncols, 16));
    return (waste >= 1.4 || (g_variant & 1048576)) ? halves : 0;
}
bool sweep8_ok(const Pass& ps, int ktiles) {
    return ktiles == 1 && !ps.twin && ps.row.expanded != ps.col.expanded && ps.epi != EPI_STORE && ps.epi != EPI_FWD && ps.epi != EPI_COS &&
           !(g_variant & 65536);
}
// (k_sweep2g also needs two candidates in the chunk: chunk_kind)
bool sweep2g_ok(const Pass& ps, int ktiles) {
    return ps.col.expanded && !ps.row.expanded && ktiles >= 16 && ps.o_bs == 0 && ps.o_nbs == 0 && ps.epi != EPI_COS;
}

int plan_sweep(const Ctx& c, const Pass& ps, SweepPlan& pl) {
    pl = SweepPlan{};
    const int esz = pl.esz = ps.i8 ? 1 : 4;
    const int Kp = pl.Kp = (int)rup(ps.K, 64 / esz);          // 64-byte k-tiles
    const int ktiles = Kp * esz / SW_BKB;
    const long K64 = rup(ps.K, 64);
    const bool cosm = ps.epi == EPI_COS, i8v2 = ps.i8 && !g_force_v1;
    const bool one_expanded = ps.row.expanded != ps.col.expanded, plain_out = ps.o_bs == 0 && ps.o_nbs == 0;
    // whole 32-column groups inside one scale block / one score block (the partial-sum table of the fast sweeps), whole 64-row
    // tiles inside both (the stationary sweeps)
    const bool scale32 = ps.sb_mode != 1 || ps.s_cs == 1 || ps.sb_div % 32 == 0;
    const bool score32 = ps.j_mode == 0 || (ps.j_mode == 1 && (ps.nj == 1 || ps.j_div % 32 == 0));
    const bool blocks64 = (ps.s_cs == 1 || ps.sb_div % 64 == 0) && (ps.j_mode == 0 || (ps.j_mode == 1 && (ps.nj == 1 || ps.j_div % 64 == 0)));
    // -- the family, in the order of the table in DESIGN.md s5 --
    // k_bound, stage B1 (one candidate over all samples): rows = samples, columns = features of a plain [M][N] layer
    const bool bound = ps.bound_kernel && i8v2 && !ps.twin && ps.Z == 1 && !ps.stores() && !cosm && plain_out && ps.bias_axis == 0 &&
                       (ps.sb_mode == 0 || ps.sb_mode == 1) && score32 && scale32 && (ps.eq_n == 1 || ps.crange);
    // k_sweep6 / k_sweep5, stationary operand: Linear layers whose invariant operand tile (128 x K int8) fits in LDS; in registers
    // (k_sweep6) for the K that sweep6_supported lists
    const bool stat_ok = !bound && !ps.stores() && i8v2 && !ps.twin && (!cosm || ps.cos6) && !(g_variant & 4) && ps.Z == 1 &&
                         ps.sb_mode == 1 && blocks64 && one_expanded && K64 <= 768 && plain_out;
    const bool regs6 = stat_ok && sweep6_supported(ktiles);
    if (ps.cos6 && !regs6) return fail(P4V_ERR_UNSUPPORTED, "cosine pass planned for k_sweep6 does not qualify for it");
    // k_sweep7 (large K): rows = samples, columns = output features of a plain [M][N] layer; features contiguous in
    // raw_out / raw_grad and a multiple of 32 (dwordx4 epilogue loads, whole 32-feature blocks), every 32-feature block
    // inside one scale / score block, exactly one operand candidate-expanded, the twin's second plane not expanded
    const bool big7 = !bound && !stat_ok && !ps.stores() && i8v2 && (!cosm || ps.cos7) && !(g_variant & 32768) && ps.Z == 1 &&
                      K64 >= 1024 && K64 % 256 == 0 && (long)ps.Mrows * ps.o_ms * 4 < (1L << 32) && ps.sb_mode == 1 && scale32 && score32 &&
                      one_expanded && !(ps.twin && (ps.row.expanded || ps.row2.expanded)) &&
                      plain_out && ps.o_ns == 1 && ps.Ncols % 32 == 0 && ps.o_ms % 4 == 0 &&
                      (c.dry || ((((unsigned long long)ps.O) | ((unsigned long long)(ps.G ? ps.G : ps.O))) & 15) == 0) && ps.bias_axis == 0;
    if (ps.cos7 && (!big7 || ps.twin)) return fail(P4V_ERR_UNSUPPORTED, "cosine pass planned for k_sweep7 does not qualify for it");
    // the fast tiled sweeps (k_sweep2 and its kin); tuning 12 = 7 keeps the cosine on the generic kernel
    const bool fast = !stat_ok && i8v2 && !cosm && scale32 && (score32 || ps.j_mode == 2);
    pl.fast_cos = cosm && !stat_ok && !big7 && i8v2 && !ps.stores() && tune(TUNE_B1_PATH) != 7 && scale32;
    pl.pairs = stat_ok && !regs6;
    pl.merged7 = big7 && ps.twin && ps.twin_disjoint && !(g_variant & 2097152);   // (variant 2097152 keeps the two-plane kernel)
    pl.kind = bound ? SK_BOUND : regs6 ? SK_SWEEP6 : stat_ok ? SK_SWEEP5 :
              big7 ? (pl.merged7 ? SK_SWEEP7_MERGED : ps.twin ? SK_SWEEP7_TWIN : SK_SWEEP7) :
              !(fast || pl.fast_cos) ? (ps.i8 ? SK_GENERIC_I8 : SK_GENERIC_F32) :
              (fast && sweep8_ok(ps, ktiles)) ? SK_SWEEP8 : (fast && sweep2g_ok(ps, ktiles)) ? SK_SWEEP2G : SK_SWEEP2;
    // per-score-block candidate ranges: the weight search on k_sweep6 (a streaming 64-row tile lies in one scale block = one score
    // block: blocks64), and the head-wise searches of the attention matmuls (score block = z % heads: a workgroup works on one z);
    // tuning 12 = 9 switches them off (A/B)
    const bool blk_ranges = ps.crange && ps.crange_blk && tune(TUNE_B1_PATH) != 9;
    pl.rblk = (blk_ranges && regs6 && !ps.row.expanded && ps.j_mode == 1 && ps.nj == ps.s_cs && ps.j_div == ps.sb_div) ? ps.crange_blk : nullptr;
    pl.rblk_z = (blk_ranges && !stat_ok && ps.j_mode == 2 && ps.nj == ps.j_div && ps.Z > 1 && !cosm && !ps.stores() && !bound && K64 < 1024)
                    ? ps.crange_blk : nullptr;
    // -- operands and planes --
    // k_sweep6 tiles the stationary operand (the one that is NOT candidate-expanded) in 256-row slabs
    const int Mp = pl.Mp = (int)rup(ps.Mrows, big7 ? (ps.twin ? 128 : 256) : (regs6 && !ps.row.expanded) ? 256 : SW_BM);
    const int Np = pl.Np = (int)rup(ps.Ncols, big7 ? 256 : (regs6 && !ps.col.expanded) ? 256 : SW_BM);
    // rows of the column operand's plane: the tile-padded count, except for the 64-column operands of the batched k_sweep2 passes
    // (attn.v: B = V, N = head_dim = 64): k_sweep2 re-reads rows 0..63 for the tile's upper half
    pl.b64 = fast && !big7 && !bound && ps.Z > 1 && !ps.col_zs_shared && ps.Ncols <= 64 && ktiles >= 2 && ktiles <= 15 && !ps.stores();
    pl.NpB = pl.b64 ? 64 : Np;
    pl.row_plane1 = (long)(ps.row_zs_shared ? 1 : ps.Z) * Mp * Kp * esz;
    pl.col_plane1 = (long)(ps.col_zs_shared ? 1 : ps.Z) * pl.NpB * Kp * esz;
    pl.exp_plane = ps.row.expanded ? pl.row_plane1 : pl.col_plane1;
    pl.chunk = (int)std::max<long>(1, std::min<long>(ps.eq_n, PLANE_BUDGET / std::max<long>(1, pl.exp_plane)));
    if (pl.pairs && pl.chunk > 1) pl.chunk &= ~1;                          // chunks start on a candidate pair
    pl.chunk_al = pl.pairs ? ((pl.chunk + 1) & ~1) : pl.chunk;             // an odd count is padded to a whole pair
    pl.slack = stat_ok ? 4096 : 0;   // the stationary sweeps' rings keep issuing a few tiles past the last candidate
    // k_sweep6 / k_sweep5 stream [row][candidate][K] / [row][pair][K]; k_sweep6's stationary operand and both operands of k_bound
    // (one candidate each) are in MFMA-fragment order
    pl.cin_exp = bound ? 3 : stat_ok ? (pl.pairs ? 2 : 1) : 0;
    pl.cin_fix = (bound || regs6) ? 3 : 0;
    pl.zero_bias_n = stat_ok ? (size_t)std::max(Mp, Np) : 0;
    pl.epi7_n = big7 ? (size_t)Mp * Np * 2 : 0;
    // k_sweep6: epilogue operands in fragment order, one image per 256 x 64 tile (8 bytes per output element) -- only where the
    // in-place gather is uncoalesced: the activation search, whose tile is transposed; in the weight search the lanes of a load
    // already read consecutive features
    const bool a_search = pl.a_search = ps.row.expanded;
    pl.s6_stiles = (a_search ? Np : Mp) / 256; pl.s6_ttiles = (int)cdiv(a_search ? ps.Mrows : ps.Ncols, 64);
    pl.epi6_on = regs6 && (a_search || ps.cos6 || tune(TUNE_EPI6W) == 1);
    pl.epi6_bytes = pl.epi6_on ? (size_t)pl.s6_stiles * pl.s6_ttiles * (256 * 64 * 8) : 0;
    // -- the partial-sum table --
    // k_sweep5 / k_sweep6: [slabs of 64 stationary rows][groups of 32 streaming rows]; k_sweep7: one row per (sample tile, wave
    // column); the tiled sweeps: [64-row slab][column], columns in groups of 32 on the fast ones
    const int MT = Mp / 64, s3_slabs = (a_search ? Np : Mp) / 64, s3_groups = pl.s3_groups = (a_search ? Mp : Np) / 32;
    const int NpP = pl.NpP = stat_ok ? s3_groups : fast ? Np / 32 : Np;
    const int MT7 = big7 ? (Mp / (ps.twin ? 128 : 256)) * 4 : 0;
    // cosine on k_sweep6: k_finish_cos's table [64-feature slab][padded sample][3]; the samples are the streaming rows of the
    // activation search (tiles of 64) and the stationary rows of the weight search (slabs of 256)
    // ... on k_sweep7: slabs of 128 features (a wave's rows), the samples are the tile-padded rows
    const bool cosp = ps.cos6 || ps.cos7;
    const int cos_slab = ps.cos7 ? 128 : 64;
    const int cos6_Sp = pl.cos6_Sp = ps.cos7 ? Mp : ps.cos6 ? (a_search ? (int)cdiv(ps.Mrows, 64) * 64 : Mp) : 0;
    const int cos6_slabs = ps.cos7 ? Np / 128 : ps.cos6 ? (a_search ? Np / 64 : (int)cdiv(ps.Ncols, 64)) : 0;
    pl.p_zs = cosp ? (long)cos6_slabs * cos6_Sp * 3 : stat_ok ? (long)s3_slabs * s3_groups : big7 ? (long)MT7 * NpP : (long)MT * NpP * (cosm ? 3 : 1);
    pl.p_cs = pl.part_cs = pl.p_zs * ps.Z;
    // k_sweep9 (before k_sweep8 in the order of the families) writes [C][Z][halves * SW9_NW] into the table allocated for the
    // 128-tile layout, where that holds it
    if (fast && !bound && !big7 && !ps.stores() && (ps.j_mode == 0 || ps.j_mode == 2)) {
        const int h9 = sweep9_halves(ps, ktiles);
        if (h9 > 0 && (long)h9 * SW9_NW <= pl.p_zs) { pl.kind = SK_SWEEP9; pl.h9 = h9; pl.p_zs = (long)h9 * SW9_NW; pl.p_cs = pl.p_zs * ps.Z; }
    }
    // -- the finish --
    pl.fin_zs = pl.p_zs;
    if (pl.kind == SK_SWEEP9) {
        pl.fin_ld = pl.fin_cols = (int)pl.p_zs; pl.fin_rows = 1; pl.fin_jdiv = std::max(1, ps.j_div);
    } else if (!cosm) {
        // k_sweep5 / k_sweep6 activation search (j_mode 0) sums the whole table; its columns are sample groups
        // (k_sweep6 skips streaming tiles that are pure padding: their table entries are never written)
        pl.fin_ld = NpP; pl.fin_rows = stat_ok ? s3_slabs : big7 ? MT7 : MT;
        pl.fin_cols = stat_ok ? (a_search ? (regs6 ? 2 * cdiv(ps.Mrows, 64) : s3_groups) : cdiv(ps.Ncols, 32)) : fast ? cdiv(ps.Ncols, 32) : ps.Ncols;
        pl.fin_jdiv = std::max(1, (fast || stat_ok) && ps.j_mode == 1 ? cdiv(ps.j_div, 32) : ps.j_div);
    } else {
        // part layout [C][ZB][ZV][FS][Sp][3] with z = zb*ZV + zv
        // (k_sweep6 / k_sweep7: Z = 1, the V blocks are consecutive runs of feature slabs of the one table; samples = the rows;
        // a V block = sb_div features = sb_div / slab whole slabs, whatever the padding behind the last block)
        const int FS = !cosp ? 0 : ps.cos_ZV == 1 ? cos6_slabs : ps.sb_div / cos_slab;
        if (cosp) pl.fin_zs = (long)FS * cos6_Sp * 3;
        pl.fin_ld = cosp ? cos6_Sp : Np; pl.fin_rows = cosp ? FS : MT; pl.fin_cols = cosp ? ps.Mrows : ps.Ncols;
        pl.fin_jdiv = std::max(1, ps.cos_j_div);
    }
    return 0;
}
// what waits for the chunk: k_sweep2g works on candidate pairs, a single candidate goes to k_sweep2
inline SweepKind chunk_kind(const SweepPlan& pl, int nc) { return (pl.kind == SK_SWEEP2G && nc < 2) ? SK_SWEEP2 : pl.kind; }

// ---- the steps of a pass ------------------------------------------------------------------------------------------------------
struct PassBufs {
    char* row; char* row2; char* col;
    float* part; float* S1; float* S2; float* scores; float* zero_bias; float* epi7; float* epi6;
    PlaneCache* pc; EpiCache* ec;
};
int pass_workspace(Ctx& c, const Pass& ps, const SweepPlan& pl, PassBufs& b) {
    // (planes above PLANE_CACHE_MAX are re-packed every pass: with three search streams and two searched operands per
    // module the cache would otherwise add up to 6 x PLANE_BUDGET of workspace on the 128-image configurations)
    PlaneCache* pc = b.pc = (ps.cache && pl.chunk >= ps.eq_n && !ps.stores() && ps.row.expanded != ps.col.expanded &&
                             !(ps.twin && ps.row2.expanded) && pl.exp_plane * (long)ps.eq_n <= PLANE_CACHE_MAX) ? ps.cache : nullptr;
    if (pc && !pc->assigned) {
        pc->buf = c.ws.get_top((size_t)pl.exp_plane * pl.chunk_al + pl.slack);
        pc->done = reinterpret_cast<unsigned char*>(c.ws.get_top((size_t)rup(ps.eq_n, 256)));
        pc->assigned = true; pc->valid = false;
        if (!c.dry && pc->done) CHK(q_fill(c, pc->done, 0, (size_t)ps.eq_n));
    }
    b.row = ps.row.prepacked ? (char*)ps.row.plane :
            (pc && ps.row.expanded) ? pc->buf : c.ws.get<char>((size_t)pl.row_plane1 * (ps.row.expanded ? pl.chunk_al : 1) + pl.slack);
    b.row2 = !ps.twin ? nullptr : ps.row2.prepacked ? (char*)ps.row2.plane : c.ws.get<char>((size_t)pl.row_plane1 * (ps.row2.expanded ? pl.chunk : 1));
    b.col = ps.col.prepacked ? (char*)ps.col.plane :
            (pc && ps.col.expanded) ? pc->buf : c.ws.get<char>((size_t)pl.col_plane1 * (ps.col.expanded ? pl.chunk_al : 1) + pl.slack);
    b.part = c.ws.get<float>((size_t)pl.part_cs * ps.eq_n);
    b.S1 = !ps.use_s1 ? nullptr : ps.S1_pre ? ps.S1_pre : c.ws.get<float>((size_t)ps.eq_n * ps.s_cs);
    b.S2 = !(ps.use_s1 && ps.twin) ? nullptr : ps.S2_pre ? ps.S2_pre : c.ws.get<float>((size_t)ps.eq_n * ps.s_cs);
    b.scores = ps.scores_keep ? ps.scores_keep : c.ws.get<float>((size_t)ps.eq_n * std::max(1, ps.nj));
    b.zero_bias = (pl.zero_bias_n && !ps.bias) ? c.ws.get<float>(pl.zero_bias_n) : nullptr;
    b.epi7 = pl.epi7_n ? c.ws.get<float>(pl.epi7_n) : nullptr;
    EpiCache* ec = b.ec = (pl.epi6_on && ps.ecache && (long)pl.epi6_bytes <= PLANE_CACHE_MAX) ? ps.ecache : nullptr;
    if (ec && !ec->assigned) {
        ec->buf = c.ws.get_top(pl.epi6_bytes);
        ec->assigned = true; ec->valid = false;
    }
    b.epi6 = !pl.epi6_on ? nullptr : ec ? reinterpret_cast<float*>(ec->buf) : c.ws.get<float>(pl.epi6_bytes / 4);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    return 0;
}

// one operand of the pass (the row side: ps.row / ps.row2 / the merged twin plane; `col`: ps.col) into `buf`: its fixed plane, or the
// candidates [c0, c0 + nc) of an expanded one
int pack_operand(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b, const Operand& op, char* buf, bool col, int c0, int nc) {
    PackParams pk = op.pk;
    pk.Rp = col ? pl.NpB : pl.Mp; pk.Kp = pl.Kp; pk.dst = buf;
    pk.Z = (col ? ps.col_zs_shared : ps.row_zs_shared) ? 1 : ps.Z;
    pk.C = op.expanded ? nc : 1;
    pk.c_inner = op.expanded ? pl.cin_exp : pl.cin_fix;
    if (op.expanded && pk.scales) pk.scales += (long)c0 * pk.sc_cs;
    if (op.expanded && ps.crange) {       // pruned pass: only the candidate groups in range, and not the ones already kept
        pk.crange = ps.crange; pk.c_base = c0;
        pk.done = (b.pc && b.pc->done) ? b.pc->done : nullptr;
    }
    // what the host knows of the range (stages A2 / B2: the survivor range it read back; stage B1: its length)
    int live_max = -1;
    if (pk.crange && ps.host_hi > ps.host_lo) live_max = std::max(0, std::min(ps.host_hi, c0 + nc) - std::max(ps.host_lo, c0));
    else if (pk.crange && ps.host_len > 0) live_max = std::min(ps.host_len, nc);
    // (the finish of this pass flags the groups as packed: FinishParams.mark_done)
    return ps.i8 ? launch_pack<int8_t>(c, pk, live_max) : launch_pack<float>(c, pk, live_max);
}
// the expanded operand's candidates [c0, c0 + nc), unless the module's plane cache holds them
int pack_expanded(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b, int c0, int nc) {
    PlaneCache* pc = b.pc;
    const bool packed = pc && pc->valid;   // (a cached plane is never chunked: one iteration)
    if (ps.row.expanded && !packed) CHK(pack_operand(c, ps, pl, b, ps.row, b.row, false, c0, nc));
    if (ps.twin && ps.row2.expanded) CHK(pack_operand(c, ps, pl, b, ps.row2, b.row2, false, c0, nc));
    if (ps.col.expanded && !packed) CHK(pack_operand(c, ps, pl, b, ps.col, b.col, true, c0, nc));
    if (pc && !ps.crange && !packed) {   // every candidate is in the buffer now (a pruned pass packs a range and keeps flags)
        pc->valid = true;
        if (!c.dry && pc->done) CHK(q_fill(c, pc->done, 1, (size_t)ps.eq_n));
    }
    return 0;
}

// the epilogue operands of k_sweep6 / k_sweep7 in fragment order, and the stationary sweeps' stand-in for a missing bias
int prep_epilogue(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b) {
    const bool a_search = pl.a_search;
    const size_t zero_bytes = sizeof(float) * pl.zero_bias_n;
    if (pl.epi6_on && !c.dry && !(b.ec && b.ec->valid)) {
        PrepEpi6Params pe{};
        pe.O = ps.O; pe.Wt = ps.G ? ps.G : ps.O; pe.bias = ps.bias ? ps.bias : b.zero_bias;
        pe.o_ss = a_search ? ps.o_ns : ps.o_ms; pe.o_ts = a_search ? ps.o_ms : ps.o_ns;
        pe.SR = a_search ? ps.Ncols : ps.Mrows; pe.TR = a_search ? ps.Mrows : ps.Ncols;
        pe.bias_on_t = a_search ? 0 : 1; pe.wt_mode = ps.cos6 ? 4 : ps.wt_mode;
        pe.stiles = pl.s6_stiles; pe.ttiles = pl.s6_ttiles; pe.E = b.epi6; pe.transposed = (ps.cos6 && !a_search) ? 1 : 0;
        if (b.zero_bias) CHK(q_fill(c, b.zero_bias, 0, zero_bytes));
        CHK(enqueue(c, KERN(PrepEpi6Params, k_prep_epi6), dim3((unsigned)std::min<long>((long)pl.s6_stiles * pl.s6_ttiles, 256L * 32)), dim3(256), 0, pe));
    }
    if (b.ec) b.ec->valid = true;
    if (pl.epi7_n && !c.dry) {
        PrepEpiParams pe{ps.O, ps.G ? ps.G : ps.O, ps.bias, ps.o_ms, ps.Mrows, ps.Ncols, ps.cos7 ? 4 : ps.wt_mode,
                         pl.Np / 256, pl.Mp / (ps.twin ? 128 : 256), ps.twin ? 1 : 0, b.epi7};
        const long chunks = (long)pl.Mp * pl.Np * 2 / 4;
        CHK(enqueue(c, KERN(PrepEpiParams, k_prep_epi), dim3((unsigned)std::min<long>(cdiv(chunks, 256), 256L * 16)), dim3(256), 0, pe));
    }
    // (with the image built above this is the second fill of the same buffer: DESIGN.md s10-7)
    if (b.zero_bias && !c.dry) CHK(q_fill(c, b.zero_bias, 0, zero_bytes));
    return 0;
}

// the planes that do not depend on the candidate, once
int pack_fixed_planes(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b) {
    if (ps.row.prepacked) {
        // prepacked row operand (the fused MLP forward): its plane(s) are on the stream already
        if (ps.row.expanded || pl.merged7 || pl.cin_fix != 0 || (ps.twin && (!ps.row2.prepacked || ps.row2.expanded)))
            return fail(P4V_ERR_INVALID, "prepacked row operand: fixed row-major plane(s) of a forward pass only");
    } else if (pl.merged7) {
        Operand both = ps.row;              // positive range: scale + upper clamp; negative range: fixed scale + lower clamp
        both.pk.mode = PACK_TWIN_I8;
        both.pk.lo = ps.row2.pk.lo; both.pk.neg_scale = ps.row2.pk.neg_scale;
        both.pk.dst2 = b.row2;              // ... where the interval is not > 0: the two planes apart (k_pack_twin), for the two-plane sweep
        CHK(pack_operand(c, ps, pl, b, both, b.row, false, 0, 1));
    } else if (ps.twin && ps.i8 && !ps.row.expanded && !ps.row2.expanded && dual_pack_ok(ps.row.pk, ps.row2.pk)) {
        // both planes of the twin row operand from one read of the source (k_pack_dual)
        PackParams p1 = ps.row.pk, p2 = ps.row2.pk;
        p1.Rp = p2.Rp = pl.Mp; p1.Kp = p2.Kp = pl.Kp; p1.Z = p2.Z = ps.row_zs_shared ? 1 : ps.Z; p1.C = p2.C = 1;
        p1.dst = b.row; p2.dst = b.row2;
        if (!c.dry) {
            const long total = (long)p1.Z * pl.Mp * (pl.Kp / 16);
            if (total >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "operand plane too large for k_pack_dual (%ld 16-element runs)", total);
            CHK(enqueue(c, KERN(PackDualParams, k_pack_dual), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 64)), dim3(256), 0, PackDualParams{p1, p2}));
        }
    } else {
        if (!ps.row.expanded) CHK(pack_operand(c, ps, pl, b, ps.row, b.row, false, 0, 1));
        if (ps.twin && !ps.row2.expanded) CHK(pack_operand(c, ps, pl, b, ps.row2, b.row2, false, 0, 1));
    }
    if (ps.col.prepacked) {
        // prepacked column operand (the fused qkv forward: v), under the row side's refusals
        if (ps.col.expanded || pl.cin_fix != 0 || !ps.i8 || !ps.stores())
            return fail(P4V_ERR_INVALID, "prepacked column operand: the fixed row-major int8 plane of a forward pass only");
    } else if (!ps.col.expanded) CHK(pack_operand(c, ps, pl, b, ps.col, b.col, true, 0, 1));
    return 0;
}

// roofline step only: g_exec_frac = how many of the chunk's candidates [c0, c0 + nc) a pruned pass runs.
// From what the host knows WITHOUT another round trip wherever it does -- the timed calibration must make the same launches, in
// the same issue rounds, as an untimed one (inside a group an extra synchronisation regroups the members): the survivor range the
// pruned pass read back anyway (stages A2 / B2 under the pass memo), or "one candidate" (stage B1 of a single score block: the
// range holds the slice winner).  Only a caller without either reads the range back here.
int chunk_exec_frac(Ctx& c, const Pass& ps, const SweepPlan& pl, int c0, int nc) {
    g_exec_frac = 1.0;
    if (!(g_stat_on && ps.crange && !c.dry)) return 0;
    int h[2] = {0, 0};
    const bool host_knows = ps.host_hi > ps.host_lo;
    const bool one_cand = !host_knows && ps.host_len == 1;        // (stage_b1_pass: the range holds the slice winner)
    if (host_knows) { h[0] = ps.host_lo; h[1] = ps.host_hi; }
    else if (one_cand) { h[0] = c0; h[1] = c0 + 1; }
    else { CHK(q_d2h(c, h, ps.crange, sizeof h)); CHK(q_sync(c)); }
    const int lo = std::max(h[0], c0), hi = std::min(h[1], c0 + nc);
    g_exec_frac = (double)std::max(0, hi - lo) / (double)nc;
    const int* blk = pl.rblk ? pl.rblk : pl.rblk_z;
    if (blk && ps.nj <= 64 && !one_cand) {               // equal-sized score blocks, each on its own range
        int hb[128];
        if (host_knows && ps.host_rblk && ps.nj <= MIR_BLK) std::copy(ps.host_rblk, ps.host_rblk + 2 * ps.nj, hb);
        else { CHK(q_d2h(c, hb, blk, sizeof(int) * 2 * ps.nj)); CHK(q_sync(c)); }
        double sum = 0;
        for (int j = 0; j < ps.nj; ++j) sum += std::max(0, std::min(std::min(hb[2 * j + 1], h[1]), c0 + nc) - std::max(std::max(hb[2 * j], h[0]), c0));
        g_exec_frac = sum / ((double)nc * ps.nj);
    }
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] pruned stage: candidates [%d, %d) of %d  (M %d N %d K %d Z %d nj %d)\n", h[0], h[1], ps.eq_n, ps.Mrows, ps.Ncols, ps.K, ps.Z, ps.nj);
    return 0;
}

// k_sweep6 / k_sweep5 over the candidates [c0, c0 + nc)
int sweep_chunk_stationary(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b, int c0, int nc) {
    const bool a_search = pl.a_search;
    const int Kp = pl.Kp;
    Sweep3Params q{};
    q.S = a_search ? b.col : b.row; q.s_zs = 0;
    q.T = a_search ? b.row : b.col; q.t_cs = 0; q.t_zs = 0;
    q.t_rs = (long)(pl.pairs ? ((nc + 1) & ~1) : nc) * Kp;   // [row][candidate][K] layout written by k_pack (c_inner)
    q.ldk = Kp; q.ktiles = Kp / SW_BKB;
    q.S1 = b.S1; q.s_cs = ps.s_cs; q.sb_on_t = a_search ? 0 : 1; q.sb_div = std::max(1, ps.sb_div);
    q.bias = ps.bias ? ps.bias : b.zero_bias; q.bias_on_t = a_search ? 0 : 1;
    q.O = ps.O; q.Wt = ps.G ? ps.G : ps.O; q.wt_mode = ps.wt_mode;
    q.o_ss = a_search ? ps.o_ns : ps.o_ms; q.o_ts = a_search ? ps.o_ms : ps.o_ns;
    q.SR = a_search ? ps.Ncols : ps.Mrows; q.TR = a_search ? ps.Mrows : ps.Ncols;
    q.c0 = c0; q.c1 = c0 + nc; q.crange = ps.crange;
    q.part = b.part; q.p_cs = pl.p_cs; q.NG = pl.s3_groups;
    q.stiles = (a_search ? pl.Np : pl.Mp) / 128; q.ttiles = (a_search ? pl.Mp : pl.Np) / 128;
    q.dbg = g_variant & 3;
    if (pl.kind == SK_SWEEP5) {
        const int cgroups = choose_cgroups((long)q.stiles * q.ttiles, nc, q.ktiles, cu_slots(c, 256, SWEEP_RECORD_KIND[SK_SWEEP5]), 30.0, 0.15);
        return launch_sweep5(c, q, ps.epi, cgroups);
    }
    // streaming tiles of 64 rows: only those holding valid rows (the plane is padded to 128)
    q.stiles = pl.s6_stiles; q.ttiles = pl.s6_ttiles; q.E = b.epi6; q.crange_blk = pl.rblk;
    const int epi6k = ps.cos6 ? (a_search ? EPI_COS : EPI_COS_T) : ps.epi;
    if (ps.cos6) q.NG = pl.cos6_Sp;
    // what the host knows of the device-side range: the launch geometry is planned for the candidates that will run
    const bool known = ps.crange && ps.host_hi > ps.host_lo;
    const int nc_known = known ? std::max(1, std::min(ps.host_hi, c0 + nc) - std::max(ps.host_lo, c0)) : nc;
    const double P6 = tune(TUNE_P6) > 0 ? 0.125 * tune(TUNE_P6) : 25.0;
    const int slots6 = cu_slots(c, 256, SWEEP_RECORD_KIND[SK_SWEEP6]);
    if (pl.rblk && known && ps.host_rblk && ps.nj <= 4) {
        // per-score-block ranges known to the host: one launch per run of OPEN blocks (a closed block -- its only survivor
        // is its stage-A winner -- has nothing to sweep: the q block of a ViT qkv layer); score block j = streaming
        // tiles [j, j + 1) * sb_div / 64 -- several blocks are whole tiles each (blocks64); ONE block need not be (96 features:
        // a tile and a half), its run ends with the last tile
        const int tpb = ps.sb_div / 64;
        for (int j = 0; j < ps.nj;) {
            if (ps.host_rblk[2 * j + 1] <= ps.host_rblk[2 * j]) { ++j; continue; }
            int j1 = j, lo = INT_MAX, hi = 0;
            double fsum = 0;
            for (; j1 < ps.nj && ps.host_rblk[2 * j1 + 1] > ps.host_rblk[2 * j1]; ++j1) {
                const int l = std::max(ps.host_rblk[2 * j1], c0), h = std::min(ps.host_rblk[2 * j1 + 1], c0 + nc);
                lo = std::min(lo, l); hi = std::max(hi, h);
                fsum += std::max(0, h - l);
            }
            Sweep3Params qq = q;
            const int tt0 = j * tpb, tt1 = j1 == ps.nj ? q.ttiles : std::min(q.ttiles, j1 * tpb);
            qq.tile0 = tt0 * q.stiles; qq.ntile = (tt1 - tt0) * q.stiles;
            const int ncr = std::max(1, hi - lo);
            g_exec_frac = fsum / ((double)(j1 - j) * nc);
            int cg6 = choose_cgroups((long)qq.ntile, ncr, q.ktiles, slots6, P6, 0.14);
            if (tune(TUNE_CG6) > 0) cg6 = std::max(1, std::min(ncr, tune(TUNE_CG6)));
            if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] sweep6 open blocks [%d, %d): tiles %d x %d ktiles %d cand %d -> cgroups %d\n", j, j1, q.stiles, tt1 - tt0, q.ktiles, ncr, cg6);
            if (hi > lo && qq.ntile > 0) CHK(launch_sweep6(c, qq, epi6k, cg6, ncr));
            j = j1;
        }
        return 0;
    }
    int cg6 = choose_cgroups((long)q.stiles * q.ttiles, nc_known, q.ktiles, slots6, P6, 0.14);
    if (tune(TUNE_CG6) > 0) cg6 = std::max(1, std::min(nc, tune(TUNE_CG6)));
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] sweep6 tiles %d x %d ktiles %d cand %d (%d known) -> cgroups %d\n", q.stiles, q.ttiles, q.ktiles, nc, nc_known, cg6);
    return launch_sweep6(c, q, epi6k, cg6, known ? nc_known : 0);
}

// k_sweep7 over the candidates [c0, c0 + nc)
int sweep_chunk_large_k(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b, int c0, int nc) {
    Sweep7Params q{};
    q.r_cs = ps.col.expanded ? pl.col_plane1 : 0;
    q.R = b.col - (long)c0 * q.r_cs;
    q.c_cs = ps.row.expanded ? pl.row_plane1 : 0;
    q.Cp = b.row - (long)c0 * q.c_cs;
    q.C2 = pl.kind == SK_SWEEP7_TWIN ? b.row2 : nullptr;
    q.ldk = pl.Kp; q.ktiles = pl.Kp / SW_BKB;
    q.S1 = b.S1; q.S2 = b.S2; q.s_cs = ps.s_cs; q.sb_div = ps.s_cs > 1 ? std::max(1, ps.sb_div) : (1 << 30);
    q.E = b.epi7;
    q.c0 = c0; q.c1 = c0 + nc; q.crange = ps.crange;
    q.part = b.part; q.p_cs = pl.p_cs; q.NG = ps.cos7 ? pl.cos6_Sp : pl.NpP;
    q.rtiles = pl.Np / 256; q.ctiles = pl.Mp / (ps.twin ? 128 : 256);
    // one workgroup per CU; per k-tile ~0.62 us (16 MFMAs per wave, two waves per SIMD), ~3 k-tiles' worth of
    // epilogue per candidate, a prologue of a few us (scale tables, first tiles)
    // (up to one candidate per workgroup: stage A of a pruned pass is 3 tiles x 100 candidates -- with the 25 groups of the
    // other sweeps 75 workgroups on 256 CUs, 140-160 us per launch)
    int cg7 = choose_cgroups((long)q.rtiles * q.ctiles, nc, q.ktiles + 3, cu_slots(c, 256, SWEEP_RECORD_KIND[ps.twin ? SK_SWEEP7_TWIN : SK_SWEEP7]), 6.0, 0.62, 100);
    if (tune(TUNE_CG7) > 0) cg7 = std::max(1, std::min(nc, tune(TUNE_CG7)));
    q.order = tune(TUNE_ORDER7) > 0 ? tune(TUNE_ORDER7) - 1 : 1;
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] sweep7 tiles %d x %d ktiles %d cand %d twin %d -> cgroups %d\n", q.rtiles, q.ctiles, q.ktiles, nc, (int)ps.twin, cg7);
    if (pl.kind == SK_SWEEP7_MERGED) { q.twin_s = ps.row.pk.scales; q.C2 = b.row2; }   // (merged or apart: decided on the device)
    return launch_sweep7(c, q, pl.kind == SK_SWEEP7_MERGED ? 2 : ps.twin ? 1 : 0, ps.epi, cg7);
}

// the tiled sweeps (k_bound, k_sweep9 / 8 / 2g / 2, the generic kernels) over the candidates [c0, c0 + nc): `kind` = chunk_kind
int sweep_chunk_tiled(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b, SweepKind kind, int c0, int nc) {
    const int esz = pl.esz, Mp = pl.Mp, Np = pl.Np, Kp = pl.Kp;
    SweepParams sp{};
    // plane pointers are biased so that the kernel can index them with the absolute candidate id
    sp.a_cs = ps.row.expanded ? pl.row_plane1 : 0;
    sp.A = b.row - (long)c0 * sp.a_cs;
    sp.a_zs = ps.row_zs_shared ? 0 : (long)Mp * Kp * esz;
    if (ps.twin) {
        sp.a2_cs = ps.row2.expanded ? pl.row_plane1 : 0;
        sp.A2 = b.row2 - (long)c0 * sp.a2_cs;
        sp.a2_zs = sp.a_zs;
    }
    sp.b_cs = ps.col.expanded ? pl.col_plane1 : 0;
    sp.B = b.col - (long)c0 * sp.b_cs;
    sp.b_zs = ps.col_zs_shared ? 0 : (long)pl.NpB * Kp * esz;
    sp.b_rows = pl.b64 ? 64 : 0;
    sp.ldk = Kp * esz; sp.ktiles = sp.ldk / SW_BKB;
    sp.S1 = b.S1; sp.S2 = b.S2; sp.s_cs = ps.s_cs; sp.sb_mode = ps.sb_mode; sp.sb_div = std::max(1, ps.sb_div);
    sp.bias = ps.bias; sp.bias_axis = ps.bias_axis; sp.bias_zs = ps.bias_zs;
    sp.O = ps.O; sp.Wt = ps.G ? ps.G : ps.O; sp.wt_mode = ps.wt_mode;
    sp.o_zs = ps.o_zs; sp.o_bs = ps.o_bs; sp.o_ms = ps.o_ms; sp.o_nbs = ps.o_nbs; sp.o_ns = ps.o_ns;
    sp.o_inner = ps.o_inner > 0 ? ps.o_inner : INT_MAX;
    sp.o_ninner = ps.o_ninner > 0 ? ps.o_ninner : INT_MAX;
    sp.M = ps.Mrows; sp.N = ps.Ncols; sp.Z = ps.Z; sp.c0 = c0; sp.c1 = c0 + nc; sp.crange = ps.crange;
    sp.crange_blk = pl.rblk_z; sp.cb_div = std::max(1, ps.j_div);
    sp.part = b.part; sp.p_cs = pl.p_cs; sp.p_zs = pl.p_zs; sp.Np = pl.NpP;
    sp.mtiles = Mp / SW_BM; sp.ntiles = Np / SW_BN;
    sp.dbg = g_variant & 3;
    sp.store = ps.store_out;
    // candidate groups: the cost model of the family (choose_cgroups), in microseconds
    const long wgs = (long)sp.mtiles * sp.ntiles * ps.Z;
    int cgroups;
    switch (kind) {
        case SK_GENERIC_I8: case SK_GENERIC_F32:
            // 2 workgroups per CU; per k-tile step ~2.6 us with fp32 operands (8 x mfma_f32_32x32x2 per 32x32 block), ~1.6 us
            // on the int8 grid (measured on the patch-embedding search)
            cgroups = choose_cgroups(wgs, nc, sp.ktiles, cu_slots(c, 512, SWEEP_RECORD_KIND[kind]), 20.0, ps.i8 ? 1.6 : 2.6);
            break;
        case SK_SWEEP9:
            sp.halves = pl.h9;
            sp.rows_p_stream = sp.a_cs == 0 ? Np : Mp;
            cgroups = choose_cgroups((long)pl.h9 * ps.Z, nc, 1, cu_slots(c, SW9_NW == 4 ? 512 : 256, SWEEP_RECORD_KIND[SK_SWEEP9]), 12.0, 0.9);
            break;
        case SK_BOUND:
            sp.bound = 1;
            sp.dbg = tune(TUNE_B1_PATH) >= 16 ? (tune(TUNE_B1_PATH) >> 4) : 0;   // (tuning 12 = 16 / 32: k_bound timing ablations)
            sp.A = b.row; sp.B = b.col; sp.a_cs = sp.b_cs = 0;   // (the fragment-order image holds the ONE candidate in range)
            [[fallthrough]];
        default:    // (the k_sweep2 model, whichever of its kin runs)
            cgroups = choose_cgroups(wgs, nc, sp.ktiles, cu_slots(c, ps.twin ? 256 : 512, SWEEP_RECORD_KIND[SK_SWEEP2]), ps.twin ? 40.0 : 25.0, ps.twin ? 0.45 : 0.40);
    }
    const bool tuned = kind != SK_GENERIC_I8 && kind != SK_GENERIC_F32 && !pl.fast_cos && !ps.stores();
    if (tuned) {
        const char* g = kind == SK_SWEEP2G ? "g" : "";
        if (const int t_ = tune(kind == SK_SWEEP2G ? TUNE_CG2G : TUNE_CG2); t_ > 0) cgroups = std::max(1, std::min(nc, t_));
        if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] sweep2%s tiles %d x %d z %d ktiles %d cand %d twin %d -> cgroups %d\n", g, sp.mtiles, sp.ntiles, ps.Z, sp.ktiles, nc, (int)ps.twin, cgroups);
    }
    return launch_sweep(c, sp, kind, ps.twin, ps.epi, cgroups);
}

// k_finish / k_finish_cos over the table as plan_sweep laid it out
int finish_pass(Ctx& c, const Pass& ps, const SweepPlan& pl, const PassBufs& b) {
    if (ps.epi == EPI_COS) {
        FinishCosParams fp{b.part, pl.p_cs, pl.fin_zs, pl.fin_ld, pl.fin_rows, ps.cos_ZB, ps.cos_ZV, pl.fin_cols, ps.eq_n,
                           ps.cos_j_mode, pl.fin_jdiv, ps.nj, ps.norm, b.scores};
        return launch_finish_cos(c, fp);
    }
    FinishParams fp{b.part, pl.p_cs, pl.fin_zs, pl.fin_ld, pl.fin_rows, ps.Z, pl.fin_cols, ps.eq_n, ps.j_mode, pl.fin_jdiv, ps.nj, ps.norm,
                    b.scores, ps.crange};
    // a pruned pass flags the candidates it packed into the module's plane
    if (ps.crange && b.pc && b.pc->done) { fp.mark_done = b.pc->done; fp.mark_n = ps.eq_n; }
    fp.crange_blk = pl.rblk ? pl.rblk : pl.rblk_z;
    return launch_finish(c, fp);
}

int run_pass(Ctx& c, Pass& ps) {
    if (ps.seg) return run_pass_seg(c, ps);
    g_alg_macs_cand = (double)ps.Mrows * ps.Ncols * ps.K * ps.Z;
    // every cached tensor read once per search pass -- both operands in fp32 as captured, raw_out and the metric weight
    g_alg_bytes = 4.0 * ((double)ps.Mrows * ps.K * (ps.row_zs_shared ? 1 : ps.Z) + (double)ps.Ncols * ps.K * (ps.col_zs_shared ? 1 : ps.Z)) +
                  (ps.G ? 8.0 : 4.0) * (double)ps.Mrows * ps.Ncols * ps.Z;
    SweepPlan pl;
    CHK(plan_sweep(c, ps, pl));
    const size_t mark = c.ws.off;
    PassBufs b{};
    CHK(pass_workspace(c, ps, pl, b));
    if (ps.pack_only) {
        // every candidate of the expanded operand into the module's plane cache, in the layout this pass's sweep streams; the
        // pass itself (and every later one of the module) then finds the plane packed
        if (b.pc && ps.row.expanded != ps.col.expanded && !ps.crange) CHK(pack_expanded(c, ps, pl, b, 0, ps.eq_n));
        c.ws.off = mark;
        return 0;
    }
    CHK(prep_epilogue(c, ps, pl, b));
    if (ps.use_s1 && !ps.s_ready) {
        ps.s1.S = b.S1; ps.s1.C = ps.eq_n; ps.s1.nblk = ps.s_cs;
        CHK(launch_scale(c, ps.s1));
        if (ps.twin) { ps.s2.S = b.S2; ps.s2.C = ps.eq_n; ps.s2.nblk = ps.s_cs; CHK(launch_scale(c, ps.s2)); }
    }
    CHK(pack_fixed_planes(c, ps, pl, b));
    for (int c0 = 0; c0 < ps.eq_n; c0 += pl.chunk) {
        const int nc = std::min(pl.chunk, ps.eq_n - c0);
        CHK(pack_expanded(c, ps, pl, b, c0, nc));
        CHK(chunk_exec_frac(c, ps, pl, c0, nc));
        const SweepKind kind = chunk_kind(pl, nc);
        if (sweep_stationary(kind)) CHK(sweep_chunk_stationary(c, ps, pl, b, c0, nc));
        else if (sweep_large_k(kind)) CHK(sweep_chunk_large_k(c, ps, pl, b, c0, nc));
        else CHK(sweep_chunk_tiled(c, ps, pl, b, kind, c0, nc));
    }
    g_exec_frac = 1.0;
    if (!ps.stores()) {
        CHK(finish_pass(c, ps, pl, b));
        if (!ps.no_select) CHK(launch_pass_select(c, ps, b.scores));
    }
    c.ws.off = mark;   // scratch of this pass is reusable by the next one (same stream => ordered)
    return 0;
}

// ---- exact candidate pruning ------------------------------------------------------------------------------------------------
// (the argument is with the prune kernels, p4v_kernels.h)  A pass becomes: stage A = all candidates on the HEAVIEST ~1/16 of
// the samples (by their share of the metric weight; its own small problem, scores only); B1 = the stage-A winners on all
// samples (the bound); B2 = the surviving range on all samples with the unpruned kernels, tiles, finish and selection --
// bit-identical totals for the survivors, hence the same selection (tests: every parity case runs with and without it,
// desc.reserved bit 3 / variant 4194304 switch it off).  Everything between the stages stays on the device.  Not used when the
// caller wants the full score tables, for the cosine metric (its terms are not one-signed), for fp32 operands other than the
// patch embedding's weight search, or where the sample slice would not be small against the whole.
// The sample slice of a module (see SliceCache): geometry, allocation (top of the workspace when the module keeps it, the bump
// region otherwise) and contents (ranking, share of the metric weight, gathered rows; only what changed is redone).
struct SliceGeo {
    bool lin; int segs, seg_rows, k /* rows per segment */, Ncols, K;
    const float* O; const float* G; int wt_mode; long o_ms;
    const float* row_src; long s_r, s_k; int zdiv; long s_z2, s_z;
    bool conv; PackParams conv_pk;     // the row operand is the im2col view of a conv input (flat: rows = (image, pixel))
    int k_cap;                         // rows per segment the buffers hold (>= k)
};
int slice_alloc(Ctx& c, SliceCache* sc, const SliceGeo& g, bool keep, bool bump) {
    if (sc->assigned) {
        if (sc->k != g.k_cap) return fail(P4V_ERR_INVALID, "slice cache reused with another geometry");
        return 0;
    }
    if (!keep && !bump) return 0;                 // a pass-local slice is allocated later, in the bump region
    const long zrows = (long)g.segs * g.seg_rows, out_elems = (long)g.segs * g.k_cap * g.Ncols, row_elems = (long)g.segs * g.k_cap * g.K;
    if (keep) {
        sc->idx = reinterpret_cast<int*>(c.ws.get_top((size_t)g.segs * g.k_cap * sizeof(int)));
        sc->mass = reinterpret_cast<float*>(c.ws.get_top((size_t)zrows * sizeof(float)));
        sc->Os = reinterpret_cast<float*>(c.ws.get_top((size_t)out_elems * sizeof(float)));
        sc->Gs = reinterpret_cast<float*>(c.ws.get_top((size_t)out_elems * sizeof(float)));
        sc->Rs = reinterpret_cast<float*>(c.ws.get_top((size_t)row_elems * sizeof(float)));
        sc->frac = reinterpret_cast<float*>(c.ws.get_top(256));
        sc->assigned = true;
    } else {
        sc->idx = c.ws.get<int>((size_t)g.segs * g.k_cap);
        sc->mass = c.ws.get<float>((size_t)zrows);
        sc->Os = c.ws.get<float>((size_t)out_elems);
        sc->Gs = c.ws.get<float>((size_t)out_elems);
        sc->Rs = c.ws.get<float>((size_t)row_elems);
    }
    sc->k = g.k_cap;
    return 0;
}
int slice_fill(Ctx& c, SliceCache* sc, const SliceGeo& g, bool host_sync_ok) {
    const long zrows = (long)g.segs * g.seg_rows;
    const void* wsrc = g.G ? (const void*)g.G : (const void*)g.O;
    const bool new_idx = sc->idx_src != wsrc || sc->idx_wt != g.wt_mode || (g.wt_mode != 1 && sc->o_src != g.O);
    if (new_idx) {
        // the heaviest rows of every segment by their share of the metric weight
        CHK(enqueue(c, KERN(RowMassParams, k_row_mass), dim3((unsigned)cdiv(zrows, 4)), dim3(256), 0, RowMassParams{g.G ? g.G : g.O, g.O, zrows, (long)g.Ncols, g.wt_mode, sc->mass}));
        CHK(enqueue(c, KERN(TopkParams, k_topk_rows), dim3(g.segs), dim3(1024), 0, TopkParams{sc->mass, g.seg_rows, g.k, sc->idx}));
        sc->idx_src = wsrc; sc->idx_wt = g.wt_mode;
        sc->o_src = sc->g_src = sc->r_src = nullptr;
        if (sc->frac && host_sync_ok && !(g_variant & 8388608)) {
            // once per module: is the slice worth it?  The bounds are as tight as the share of the metric weight the slice
            // holds (ViT class-token rows: > 0.99; the qkv layers, whose keys and values of every token feed the class token:
            // 0.72 -- still worth it, measured: 187 -> 168 ms per ViT-B calibration); below 0.5 most candidates survive and
            // the three stages cost more than the full sweep they replace -- such a module keeps the full sweep (variant
            // 8388608: always prune).  Round 6: that was measured on 6 304-row layers.  On the 128-image configurations a pass
            // is 10-200 x larger while the stages' fixed costs are the same, and Swin (no class token: the slice holds 0.1-0.25
            // of the weight) still loses a fifth of its search time to candidates the slice already rules out: from 65 536
            // sample rows on a module prunes when its slice holds 5 % (Swin-B/384 x 128: search 4.75 -> 3.83 s; 25 %: no change,
            // 1 %: 3.81 s).  What survives is re-evaluated exactly as before: the selection does not depend on the threshold.
            float f = 1.0f;
            int* hm = host_mirror(c);
            CHK(enqueue(c, KERN(MassFracParams, k_mass_fraction), dim3(1), dim3(1024), 0,
                        MassFracParams{sc->mass, zrows, sc->idx, g.segs, g.seg_rows, g.k, sc->frac, hm ? reinterpret_cast<float*>(hm + 4) : nullptr}));
            if (!hm) CHK(q_d2h(c, &f, sc->frac, sizeof f));
            CHK(q_sync(c));
            if (hm) f = *reinterpret_cast<volatile float*>(hm + 4);
            if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] slice holds %.4f of the metric weight (%d x %d of %d rows)\n", f, g.segs, g.k, g.seg_rows);
            sc->frac_host = f;
            if (g.k < g.k_cap && !(f >= 0.97f)) {      // the small slice does not hold the weight: the full one (ranked again)
                SliceGeo g2 = g;
                g2.k = g.k_cap;
                sc->idx_src = nullptr;
                return slice_fill(c, sc, g2, host_sync_ok);
            }
            const bool big_pass = zrows >= (tune(TUNE_LOOSE_ROWS) > 0 ? (long)tune(TUNE_LOOSE_ROWS) : 65536L);
            if (!(f >= (tune(TUNE_LOOSE_PCT) > 0 ? 0.01f * tune(TUNE_LOOSE_PCT) : big_pass ? 0.05f : 0.5f))) { sc->loose = true; return 0; }
        }
        sc->k_eff = g.k;
    }
    const int rows = g.segs * g.k;
    int gather_rc = 0;
    auto gather = [&](const float* src, long s0, long s3, int d3, float* dst, int seg, int zdiv, long sz2, long sz) {
        GatherParams gp{src, s0, 0, 0, s3, 1, 1, d3, sc->idx, rows, dst, seg, zdiv, sz2, sz};
        const long total = (long)rows * d3;
        if (const int r_ = enqueue(c, KERN(GatherParams, k_gather), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 16)), dim3(256), 0, gp)) gather_rc = r_;
    };
    const int seg = g.lin ? 0 : g.k;
    const long o_seg = (long)g.seg_rows * g.Ncols;                // raw_out / raw_grad: dense [Z][M][N]
    if (sc->o_src != g.O) { gather(g.O, g.o_ms, 1, g.Ncols, sc->Os, seg, 1, o_seg, 0); sc->o_src = g.O; }
    if (g.G && sc->g_src != g.G) { gather(g.G, g.o_ms, 1, g.Ncols, sc->Gs, seg, 1, o_seg, 0); sc->g_src = g.G; }
    if (sc->r_src != g.row_src) {
        if (g.conv) {
            const long total = (long)rows * g.K;
            CHK(enqueue(c, KERN(GatherIm2colParams, k_gather_im2col), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 16)), dim3(256), 0, GatherIm2colParams{g.conv_pk, sc->idx, rows, sc->Rs}));
        } else if (g.lin) gather(g.row_src, g.s_r, 1, g.K, sc->Rs, 0, 1, 0, 0);
        else gather(g.row_src, g.s_r, g.s_k, g.K, sc->Rs, g.k, g.zdiv, g.s_z2, g.s_z);
        sc->r_src = g.row_src;
        sc->aplane.valid = false;
    }
    return gather_rc;
}

// What became of a pass handed to a pruned driver = its slot of p4v_prune_counters
enum PruneOutcome { PRUNE_STAGED = 0, PRUNE_NO_SURVIVORS = 1, PRUNE_KEEP_FULL = 2, PRUNE_NOT_ELIGIBLE = 3 };
inline bool prune_switched_off() { return (g_variant & 4194304) != 0; }
struct PrunePlan {
    bool lin;                 // Z = 1 (Linear, Conv): one ranking over all samples; MatMul: one per batch entry, the column operand whole
    int segs, seg_rows;       // ranking segments, rows ranked per segment
    int k_cap, k;             // rows per segment the slice buffers hold / stage A starts on (fill_slice: what the module settled on)
    bool conv_rows;           // the row operand is the im2col view of a conv input (gathered element by element)
    SliceGeo geo, geo2;       // the slices of the two tiers
    bool tier2; int k2;       // a second, larger slice is planned (ps.scache2) and its rows
    bool virt;                // several score blocks whose entries of the candidate table are exactly one row: stage B1 on ONE synthetic candidate
    bool hull_selects;        // k_prune_hull makes the selection when nothing survives besides stage B1's candidates
    bool b1_bound;            // stage B1 is ONE candidate per score block over all samples on a layout k_bound takes
};
// k_prune_hull makes the pass's selection when nothing survives besides stage B1's candidates (its non-virt selection is serial over
// the blocks: up to 32 of them).  plan_prune and p4v_debug_prune_decide.
inline bool prune_hull_selects(bool scores_out, bool interval, bool virt, int nj) { return !scores_out && interval && (virt || nj <= 32); }
// The only place that decides whether a pass is staged and with what geometry (DESIGN.md s5.1 lists the tests in this order).
// Allocates nothing; reads the module's slice cache for what earlier passes of the module found out.
PruneOutcome plan_prune(const Ctx& c, const Pass& ps, PrunePlan& pl) {
    if (!ps.prunable || !(ps.i8 || ps.prunable_f32) || ps.epi == EPI_COS || ps.stores() || ps.scores_out || ps.best_out || ps.crange || ps.no_select) return PRUNE_NOT_ELIGIBLE;
    if (prune_switched_off() || ps.eq_n < 32 || ps.nj < 1 || ps.nj > 4096) return PRUNE_NOT_ELIGIBLE;
    // geometry of the slice.  Linear: the k heaviest of its M samples (rows of x / raw_out / raw_grad).  MatMul: the 16
    // heaviest rows (queries) of EVERY batch entry (image, head) -- the column operand stays whole.  Measured on ViT-B/224 x 32
    // (tools/row_mass.py, tools/row_mass_mm.py): 99.9 % of raw_grad^2 sits in 1/8 of a Linear's samples and 99.7-100 % in ONE
    // row of each (image, head) of the attention matmuls -- the class-token rows, the only ones the classifier reads.
    const bool lin = pl.lin = ps.Z == 1;
    pl.segs = lin ? 1 : ps.Z;
    pl.seg_rows = ps.Mrows;
    pl.conv_rows = lin && ps.row.pk.conv && ps.row.pk.Z == 1 && !ps.twin;
    if (lin) {
        pl.k_cap = (int)std::min<long>(rup(std::max(1, ps.Mrows / (tune(TUNE_SLICE_DIV) > 0 ? tune(TUNE_SLICE_DIV) : 16)), 256), rup(ps.Mrows, 256));
        if ((long)pl.k_cap * 5 > (long)ps.Mrows * 2) return PRUNE_KEEP_FULL;    // slice > 40 % of the samples: not worth the stages
        // dense row-major operands only (or the im2col rows of a conv input)
        if (ps.o_ms != ps.Ncols || ps.o_ns != 1 || ps.o_bs || ps.o_nbs || ps.row.pk.zdiv > 0 ||
            (!pl.conv_rows && (ps.row.pk.conv || ps.row.pk.s_k != 1 || ps.row.pk.s_r != ps.K))) return PRUNE_KEEP_FULL;
    } else {
        pl.k_cap = 16;
        if (ps.Mrows < 64 || ps.row_zs_shared || ps.o_zs != (long)ps.Mrows * ps.Ncols || ps.o_ms != ps.Ncols || ps.o_ns != 1 ||
            ps.o_bs || ps.o_nbs || ps.row.pk.zdiv <= 0 || ps.row.pk.conv) return PRUNE_KEEP_FULL;
    }
    if (ps.scache && ps.scache->loose) return PRUNE_KEEP_FULL;     // an earlier pass of the module measured the slice (slice_fill)
    // A Linear first tries a QUARTER of the slice: the M/64 (at least 128) heaviest samples -- in a ViT the class-token rows, one
    // per image of 197+ tokens, are among them -- hold > 97 % of the weight in every layer but qkv, and stage A costs in proportion
    // to the slice.  Measured (ViT-B/224 x 32, one box): full slice 155.4 ms per calibration, 256 rows 151.2, 128 rows 148.8,
    // 64 rows 148.6 (p4v_debug_set_tuning(11, rows) overrides the size)
    pl.k = pl.k_cap;
    if (ps.scache && ps.scache->k_eff > 0) pl.k = ps.scache->k_eff;
    else if (lin && ps.scache && ps.host_sync_ok && !c.dry && pl.k_cap >= 512 && !(g_variant & 8388608))
        pl.k = tune(TUNE_SLICE_SMALL) > 0 ? std::min(tune(TUNE_SLICE_SMALL), pl.k_cap)
                                          : (int)std::min<long>(std::max<long>(128, rup(ps.Mrows / 64, 64)), pl.k_cap / 2);
    pl.geo = SliceGeo{lin, pl.segs, pl.seg_rows, pl.k, ps.Ncols, ps.K, ps.O, ps.G, ps.wt_mode, ps.o_ms, ps.row.pk.src, ps.row.pk.s_r, ps.row.pk.s_k,
                      ps.row.pk.zdiv, ps.row.pk.s_z2, ps.row.pk.s_z, pl.conv_rows, ps.row.pk, pl.k_cap};
    // Second tier (Linear layers whose weight is spread over more samples than the first slice holds -- the qkv layers: the keys
    // and values of EVERY token feed the class token, 0.72 of the weight in their 512 heaviest samples, ~32 of 100 candidates
    // survive stage B1's bound and stage B2 swept them over all 6304 samples: 37 % of the sweep time of a ViT-B calibration):
    // the survivors are first swept over the M/4 heaviest samples (a partial sum over ANY subset of the samples is an upper
    // bound; this one is ~3 x tighter) and only what survives THAT goes to stage B2.  The buffers are planned unconditionally
    // (the dry run cannot know whether a module will need them).
    // (M / 4: measured on ViT-B/224 x 32, k_sweep6 time per calibration 30.6 ms without the tier, 29.1 / 28.1 / 28.7 / 29.4 ms with M / 3, 4, 6, 8)
    pl.k2 = (int)rup(std::max(1, ps.Mrows / (tune(TUNE_TIER2_DIV) > 0 ? tune(TUNE_TIER2_DIV) : 4)), 256);
    pl.tier2 = lin && ps.scache && ps.scache2 && !ps.row.pk.conv && tune(TUNE_TIER2) != 1 &&
               pl.k2 >= 2 * pl.k_cap && (long)pl.k2 * 5 <= (long)ps.Mrows * 2;
    pl.geo2 = pl.geo;
    pl.geo2.k = pl.geo2.k_cap = pl.k2;
    pl.virt = ps.nj > 1 && ps.cand_off == 0 && ps.cand_js * ps.nj == ps.cand_cs && ps.cand_cs <= 4096;
    pl.hull_selects = prune_hull_selects(ps.scores_out != nullptr, ps.interval != nullptr, pl.virt, ps.nj);
    // ONE candidate per score block over all samples: the kernel built for that (k_bound).
    // Its totals are summed in another order than the sweeps', so from stage B1 on nothing may depend on its numbers but the
    // bound: the selections are either "the only survivor of every block" (no totals involved) or come from stage B2, which
    // always re-evaluates stage B1's candidates together with the other survivors.  The candidate's plane is packed for this
    // pass (one candidate: ~12 us) instead of being read from the module's plane, whose layout belongs to its sweep kernel.
    pl.b1_bound = lin && ps.i8 && !ps.twin && (pl.virt || ps.nj == 1);
    return PRUNE_STAGED;
}

#define PRUNE_COUNT(i) do { if (!c.dry) g_prune_cnt[i].fetch_add(1, std::memory_order_relaxed); } while (0)
// The margin by which a stage-A (slice) score must lie below the bound L* before the candidate is dropped.  Both numbers are
// sums of same-signed terms whose per-element values are computed by the same arithmetic in every stage; what differs is the
// order of summation.  Every sweep sums in fp32 only INSIDE a wave -- at most PRUNE_FP32_CHAIN additions in a row: the 128
// outputs a lane of k_sweep7 owns per candidate (the longest chain of any sweep; k_sweep6: 32, k_sweep2/8/9: 32-48, the generic
// and k_sos_split sweeps: 64) + the 6 levels of the cross-lane reduction -- and everything across waves / tiles / slabs is
// k_finish's fp64.  A chain of n additions of same-signed fp32 terms is off by at most (n - 1) u / (1 - (n - 1) u) relative,
// u = 2^-24; the slice sum and the bound each carry one such error, so 2 n u = 1.6e-5 bounds their disagreement and the margin
// is 4 x that, never below the 1e-4 of round 3 (which is therefore what is used; a kernel with a longer fp32 chain must raise
// PRUNE_FP32_CHAIN).  Variant 134217728 cross-checks every pruned pass against the full sweep (tests).
// "The same arithmetic" is measured, stage A running on other kernels than the totals (k_slice_a / k_slice_b2 against k_sweep9,
// slice-shaped launches of the sweeps, k_sos_split on 16 rows): with raw_grad exactly zero outside the slice's rows the slice sum
// and the total are the same sum, and every pairing agrees to <= 2.4e-7 relative, 0.015 of the 1.6e-5
// (tests/test_hip_prune_premises.py, p4v_debug_prune_tables; profiles/r31_prune_premises_margins.json).
constexpr int PRUNE_FP32_CHAIN = 128 + 6;
inline float prune_margin() { return std::max(1e-4f, 4.0f * 2.0f * (float)PRUNE_FP32_CHAIN * 5.9604645e-8f); }
// The debug cross-check: `pruned_fn`, then `full_fn` -- the full sweep of the same pass into the same `interval` --; the n
// selections must be bit-identical.  A dry run plans both and compares nothing.
template <class PrunedFn, class FullFn>
int cross_checked(Ctx& c, const float* interval, int n, const char* what, PrunedFn&& pruned_fn, FullFn&& full_fn) {
    std::vector<float> pruned(n), full(n);
    CHK(pruned_fn());
    if (!c.dry) { CHK(q_d2h(c, pruned.data(), interval, sizeof(float) * n)); CHK(q_sync(c)); }
    CHK(full_fn());
    if (c.dry) return 0;
    CHK(q_d2h(c, full.data(), interval, sizeof(float) * n));
    CHK(q_sync(c));
    for (int i = 0; i < n; ++i)
        if (std::memcmp(&full[i], &pruned[i], sizeof(float)) != 0)
            return fail(P4V_ERR_INVALID, "exact candidate pruning selected another candidate than the full sweep (%s, output %d: %.9g vs %.9g)", what, i, (double)pruned[i], (double)full[i]);
    return 0;
}
// ---- stage A of a pruned MatMul B search in one kernel (k_slice_b2: B quantised in the kernel, no candidate planes) --------------
// `a` is the stage-A pass run_pass_pruned built (row operand = the 16-row slices, dense [Z][16][K]; column operand = the whole B,
// candidate-expanded); `SA` receives the scores [eq_n][nj].  Conditions: int8, head-wise scales (block = z % H on both the
// quantiser and the output scales), K <= 256, N <= 208, no bias, a difference metric.
bool slice_b_ok(const Pass& a) {
    const PackParams& b = a.col.pk;
    return a.i8 && a.col.expanded && !a.row.expanded && !(a.twin && a.row2.expanded) && a.Z > 1 && a.Mrows <= 16 && !a.stores() &&
           a.epi != EPI_COS && a.epi != EPI_STORE && a.epi != EPI_FWD && !a.bias && a.use_s1 && a.sb_mode == 2 && a.j_mode == 2 &&
           a.sb_div == a.j_div && a.s_cs == a.sb_div && !a.crange && a.scores_keep && a.no_select &&
           !b.conv && b.mode == PACK_SYM && b.blk_mode == 2 && b.blk_div == a.sb_div && b.scales && !a.col_zs_shared && !a.row_zs_shared &&
           rup(a.K, 64) <= 256 && a.Ncols <= 208 && (rup(a.K, 64) == 64 || a.Ncols <= 64) && a.o_ms == a.Ncols && a.o_ns == 1 &&
           a.o_zs == (long)a.Mrows * a.Ncols && !a.o_bs && !a.o_nbs && !g_force_v1;
}
int run_slice_b(Ctx& c, Pass& a, float* SA) {
    const int Kp = (int)rup(a.K, 64), Z = a.Z;
    const size_t mark = c.ws.off;
    int8_t* A1 = c.ws.get<int8_t>((size_t)Z * 16 * Kp);
    int8_t* A2 = a.twin ? c.ws.get<int8_t>((size_t)Z * 16 * Kp) : nullptr;
    float* part = c.ws.get<float>((size_t)a.eq_n * Z * 4);      // one float per (candidate, batch entry, wave)
    float* S1 = a.S1_pre ? a.S1_pre : c.ws.get<float>((size_t)a.eq_n * a.s_cs);
    float* S2 = !a.twin ? nullptr : a.S2_pre ? a.S2_pre : c.ws.get<float>((size_t)a.eq_n * a.s_cs);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    if (!a.s_ready) {
        a.s1.S = S1; a.s1.C = a.eq_n; a.s1.nblk = a.s_cs;
        CHK(launch_scale(c, a.s1));
        if (a.twin) { a.s2.S = S2; a.s2.C = a.eq_n; a.s2.nblk = a.s_cs; CHK(launch_scale(c, a.s2)); }
    }
    auto pack16 = [&](const Operand& op, int8_t* dst) -> int {     // the slice's fixed plane(s): [Z][16][Kp], row-major
        PackParams pk = op.pk;
        pk.Rp = 16; pk.Kp = Kp; pk.dst = dst; pk.Z = Z; pk.C = 1; pk.c_inner = 0;
        return launch_pack<int8_t>(c, pk);
    };
    CHK(pack16(a.row, A1));
    if (a.twin) CHK(pack16(a.row2, A2));
    if (!c.dry) {
        const PackParams& b = a.col.pk;
        SliceBParams kp{};
        kp.A = A1; kp.A2 = A2;
        kp.B = b.src; kp.b_z2 = b.s_z2; kp.b_z = b.s_z; kp.b_n = b.s_r; kp.b_k = b.s_k; kp.zdiv = b.zdiv;
        kp.bscale = b.scales; kp.bs_cs = b.sc_cs; kp.bs_div = b.blk_div; kp.lo = b.lo; kp.hi = b.hi;
        kp.S1 = S1; kp.S2 = S2; kp.s_cs = a.s_cs; kp.s_div = a.sb_div;
        kp.O = a.O; kp.Wt = a.G ? a.G : a.O; kp.wt_mode = a.wt_mode;
        kp.Z = Z; kp.M = a.Mrows; kp.K = a.K; kp.Kp = Kp; kp.N = a.Ncols; kp.C = a.eq_n; kp.part = part;
        const int nb = cdiv(a.Ncols, 16);
        // every wave runs every candidate of its workgroup, the prologue (B -> registers) is paid per workgroup: >= 512 workgroups
        // of >= 10 candidates (3 workgroups per CU -- 2 with the twin's second accumulator set, 250 registers: whole rounds of 256 x that)
        const int slots = std::max(8, 256 * (a.twin ? 2 : 3) / lockstep(c, 13));
        int groups = std::max(1, std::min(a.eq_n / 10, cdiv(std::max(1, 512 / lockstep(c, 13)), Z)));
        // no mostly-empty last round -- where the rounds are few (ViT: 384 batch entries; with tens of thousands of them, Swin's
        // windows, the tail does not matter and more groups only repeat the prologue)
        while ((long)Z * groups < 4L * slots && groups < a.eq_n / 10 && ((long)Z * groups) % slots != 0 && ((long)Z * groups) % slots < slots * 3 / 4) ++groups;
        if (tune(TUNE_CG2) > 0) groups = std::max(1, std::min(a.eq_n, tune(TUNE_CG2)));
        const dim3 grid(Z, groups), block(256);
        const float qbias = (b.lo == -128 && b.hi == 127 && tune(TUNE_B1_PATH) != 11) ? cvt_bias(c) : 0.0f;   // 12 = 11: quant_fast1 (A/B)
        const StatInfo si{13, 16.0 * nb * 16 * Kp * Z * a.eq_n * (a.twin ? 2 : 1), (double)a.Mrows * a.Ncols * a.K * Z * a.eq_n, g_stage, Z, groups,
                          4.0 * ((double)a.Mrows * a.K * Z + (double)a.Ncols * a.K * Z) + (a.G ? 8.0 : 4.0) * (double)a.Mrows * a.Ncols * Z};
        const StatInfo* sp = &si;
        int r_ = 0;
        SliceB2Params kp2{kp, qbias};
#define P4V_LAUNCH_SB2(TW, KTM, NBW)                                                                                                  \
        P4V_EPI4(a.epi, r_ = (qbias != 0.0f) ? enqueue(c, KERN_T(SliceB2Params, k_slice_b2, TW, KTM, NBW, E, true), grid, block, 0, kp2, sp)   \
                                             : enqueue(c, KERN_T(SliceB2Params, k_slice_b2, TW, KTM, NBW, E, false), grid, block, 0, kp2, sp); break)
        if (Kp == 64) { if (a.twin) { P4V_LAUNCH_SB2(true, 1, 4) } else { P4V_LAUNCH_SB2(false, 1, 4) } }
        else { if (a.twin) { P4V_LAUNCH_SB2(true, 4, 1) } else { P4V_LAUNCH_SB2(false, 4, 1) } }
#undef P4V_LAUNCH_SB2
        if (r_) return r_;
    }
    FinishParams fp{part, (long)Z * 4, 4L, 4, 1, Z, 4, a.eq_n, a.j_mode, std::max(1, a.j_div), a.nj, a.norm, SA, nullptr};
    CHK(launch_finish(c, fp));
    c.ws.off = mark;
    return 0;
}

// ... and of a pruned MatMul A search with K <= 64 (k_slice_a: the slice is quantised per candidate in registers, B fixed)
bool slice_a_ok(const Pass& a) {
    const PackParams& r = a.row.pk;
    return a.i8 && a.row.expanded && !a.col.expanded && !a.twin && a.Z > 1 && a.Mrows <= 16 && !a.stores() &&
           a.epi != EPI_COS && a.epi != EPI_STORE && a.epi != EPI_FWD && !a.bias && a.use_s1 && a.sb_mode == 2 && a.j_mode == 2 &&
           a.sb_div == a.j_div && a.s_cs == a.sb_div && !a.crange && a.scores_keep && a.no_select &&
           !r.conv && r.mode == PACK_SYM && r.blk_mode == 2 && r.blk_div == a.sb_div && r.scales && r.s_k == 1 && r.s_r == a.K &&
           r.zdiv > 0 && r.s_z == (long)a.Mrows * a.K && r.s_z2 == (long)r.zdiv * a.Mrows * a.K && a.Mrows == 16 &&
           !a.col_zs_shared && !a.row_zs_shared && a.K <= 64 && a.Ncols <= 208 && a.o_ms == a.Ncols && a.o_ns == 1 &&
           a.o_zs == (long)a.Mrows * a.Ncols && !a.o_bs && !a.o_nbs && !g_force_v1;
}
int run_slice_a(Ctx& c, Pass& a, float* SA) {
    const int Z = a.Z, nb = cdiv(a.Ncols, 16);
    const size_t mark = c.ws.off;
    int8_t* Bp = c.ws.get<int8_t>((size_t)Z * nb * 16 * 64);
    float* part = c.ws.get<float>((size_t)a.eq_n * Z);
    float* S1 = a.S1_pre ? a.S1_pre : c.ws.get<float>((size_t)a.eq_n * a.s_cs);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    if (!a.s_ready) {
        a.s1.S = S1; a.s1.C = a.eq_n; a.s1.nblk = a.s_cs;
        CHK(launch_scale(c, a.s1));
    }
    {
        PackParams pk = a.col.pk;                          // the fixed column operand: [Z][nb * 16][64], row-major
        pk.Rp = nb * 16; pk.Kp = 64; pk.dst = Bp; pk.Z = Z; pk.C = 1; pk.c_inner = 0;
        CHK(launch_pack<int8_t>(c, pk));
    }
    if (!c.dry) {
        const PackParams& r = a.row.pk;
        SliceAParams kp{};
        kp.A = r.src; kp.B = Bp;
        kp.ascale = r.scales; kp.as_cs = r.sc_cs; kp.as_div = r.blk_div; kp.lo = r.lo; kp.hi = r.hi;
        kp.S1 = S1; kp.s_cs = a.s_cs; kp.s_div = a.sb_div;
        kp.O = a.O; kp.Wt = a.G ? a.G : a.O; kp.wt_mode = a.wt_mode;
        kp.Z = Z; kp.M = a.Mrows; kp.K = a.K; kp.N = a.Ncols; kp.C = a.eq_n; kp.part = part;
        kp.qbias = (r.lo == -128 && r.hi == 127 && tune(TUNE_B1_PATH) != 11) ? cvt_bias(c) : 0.0f;
        const int groups = std::max(1, std::min(a.eq_n / 4, cdiv(std::max(1, 1024 / lockstep(c, 14)), Z)));
        const dim3 grid(Z, groups), block(256);
        const StatInfo si{14, 16.0 * nb * 16 * 64 * Z * a.eq_n, (double)a.Mrows * a.Ncols * a.K * Z * a.eq_n, g_stage, Z, groups,
                          4.0 * ((double)a.Mrows * a.K * Z + (double)a.Ncols * a.K * Z) + (a.G ? 8.0 : 4.0) * (double)a.Mrows * a.Ncols * Z};
        const StatInfo* sp = &si;
        P4V_EPI4(a.epi, CHK(enqueue(c, KERN_T(SliceAParams, k_slice_a, 13, E), grid, block, 0, kp, sp)); break)
    }
    FinishParams fp{part, (long)Z, 1L, 1, 1, Z, 1, a.eq_n, a.j_mode, std::max(1, a.j_div), a.nj, a.norm, SA, nullptr};
    CHK(launch_finish(c, fp));
    c.ws.off = mark;
    return 0;
}

// ---- the pieces of a pruned pass: buffers, stage passes, stage runner, survivors ------------------------------------------------
// Carved in this order -- the dry run is the workspace contract.  The module's slices at the top of the workspace (first use),
// then from `mark` on the scratch of this pass; a pass without a module slice gathers into a pass-local one behind its tables.
struct PruneBufs {
    size_t mark, tab;                    // tab: entries of one score table, [eq_n][nj]
    float *SA, *SB, *S2, *SA2;           // scores of stage A, B1, B2 and (tier 2) A2
    int *r1, *r2, *r3;                   // candidate ranges: the stage-A winners (k_prune_pick), the survivors of tier 1 and of tier 2 (k_prune_hull)
    int* best_idx;                       // virt: the stage-A winner of every score block
    int *rblk2, *rblk3;                  // per-score-block survivor ranges of the two hulls
    float* vrow;                         // virt: the synthetic candidate's row of the candidate table
    float *S1s, *S2s;                    // one scale table (twin: two) for all stages
    SliceCache local; SliceCache *sc, *sc2;
};
int prune_workspace(Ctx& c, const Pass& ps, const PrunePlan& pl, PruneBufs& b) {
    b.sc = ps.scache ? ps.scache : &b.local;
    CHK(slice_alloc(c, b.sc, pl.geo, ps.scache != nullptr, /*bump=*/false));
    b.sc2 = pl.tier2 ? ps.scache2 : nullptr;
    if (b.sc2) CHK(slice_alloc(c, b.sc2, pl.geo2, true, /*bump=*/false));
    b.mark = c.ws.off;
    b.tab = (size_t)ps.eq_n * ps.nj;
    b.SA = c.ws.get<float>(b.tab);
    b.SB = c.ws.get<float>(b.tab);
    b.S2 = c.ws.get<float>(b.tab);
    b.SA2 = b.sc2 ? c.ws.get<float>(b.tab) : nullptr;
    b.r1 = c.ws.get<int>(6);
    b.r2 = b.r1 + 2;
    b.r3 = b.r1 + 4;
    b.best_idx = c.ws.get<int>((size_t)ps.nj);
    b.rblk2 = c.ws.get<int>((size_t)4 * ps.nj);
    b.rblk3 = b.rblk2 + 2 * ps.nj;
    b.vrow = c.ws.get<float>((size_t)std::max(1, ps.cand_cs));
    b.S1s = ps.use_s1 ? c.ws.get<float>((size_t)ps.eq_n * ps.s_cs) : nullptr;
    b.S2s = (ps.use_s1 && ps.twin) ? c.ws.get<float>((size_t)ps.eq_n * ps.s_cs) : nullptr;
    if (!ps.scache) CHK(slice_alloc(c, b.sc, pl.geo, false, /*bump=*/true));
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    return 0;
}
// The slice's contents (slice_fill: only what changed is redone).  The first pruned pass of a module measures the share of the
// metric weight its slice holds: a quarter slice that does not hold it gives way to the full one (pl.k follows what the module
// settled on), and a slice that turns out loose hands the pass back to the full sweep -- PRUNE_KEEP_FULL, the buffers released.
int fill_slice(Ctx& c, const Pass& ps, PrunePlan& pl, PruneBufs& b, PruneOutcome& outcome) {
    if (c.dry) return 0;
    CHK(slice_fill(c, b.sc, pl.geo, ps.host_sync_ok));
    if (b.sc->loose) { c.ws.off = b.mark; outcome = PRUNE_KEEP_FULL; return 0; }
    if (b.sc->k_eff > 0) pl.k = b.sc->k_eff;
    return 0;
}

// the row operand of a stage that runs on a slice: the gathered rows, dense [segment][k][K]
inline void slice_rows(PackParams& pk, const float* rows, int k, int K, bool lin) {
    pk.src = rows; pk.R = k; pk.s_k = 1; pk.s_r = K; pk.conv = 0;
    if (!lin) { pk.s_z = (long)k * K; pk.s_z2 = (long)pk.zdiv * k * K; }
}
// every stage reads the same scale tables; stage A (or B1 on its synthetic candidate) computes them, `ready`: they are there
inline void shared_scales(Pass& p, const PruneBufs& b, bool ready) { p.S1_pre = b.S1s; p.S2_pre = b.S2s; p.s_ready = ready; }
// A survivor range as the host read it (read_survivors); all zero: the host does not know it
struct Survivors { int lo = 0, hi = 0, count = 0; int blk[2 * MIR_BLK] = {}; bool blk_known = false; };
// a stage on a device-side candidate range, with what the host knows of it (`s` must outlive the pass)
inline void ranged(Pass& p, const int* crange, const int* crange_blk, const Survivors& s) {
    p.crange = crange; p.crange_blk = crange_blk;
    p.host_lo = s.lo; p.host_hi = s.hi; p.host_rblk = s.blk_known ? s.blk : nullptr;
}
// Stages A / A2: `ps` on k gathered rows per segment of the row operand, raw_out and raw_grad; scores only.
// The candidate-expanded plane of the module is shared with the stage when the slice leaves that operand whole (the column
// operand: weights of a Linear, B of a matmul): stage A packs all candidates into the module's plane cache once, the later
// stages and rounds find them there -- as the unpruned passes do -- and when it is the sliced operand that is expanded
// (activation search), its slice plane is kept with the slice.
Pass slice_stage_pass(const Pass& ps, const PrunePlan& pl, SliceCache* sc, int k, float* scores) {
    Pass a = ps;
    a.O = sc->Os; a.G = ps.G ? sc->Gs : nullptr;
    a.Mrows = k;
    slice_rows(a.row.pk, sc->Rs, k, ps.K, pl.lin);
    if (ps.twin) slice_rows(a.row2.pk, sc->Rs, k, ps.K, pl.lin);
    if (!pl.lin) a.o_zs = (long)k * ps.Ncols;
    a.cache = ps.col.expanded ? ps.cache : (ps.cache && ps.scache) ? &sc->aplane : nullptr;
    a.ecache = nullptr; a.scores_keep = scores; a.no_select = true;
    return a;
}
// stage A: all candidates on the slice
Pass stage_a_pass(const Pass& ps, const PrunePlan& pl, const PruneBufs& b) {
    Pass a = slice_stage_pass(ps, pl, b.sc, pl.k, b.SA);
    shared_scales(a, b, false);
    return a;
}
// stage B1: the stage-A winners on all samples -> the bound
Pass stage_b1_pass(const Pass& ps, const PrunePlan& pl, const PruneBufs& b) {
    Pass b1 = ps;
    b1.scores_keep = b.SB; b1.no_select = true;
    if (pl.virt) {              // ONE candidate, its row of the table written by k_prune_pick: whatever read the table reads that row
        b1.eq_n = 1; b1.cache = nullptr;
        auto swap = [&](const float*& ptr) { if (ptr == ps.cands) ptr = b.vrow; };
        swap(b1.row.pk.scales); swap(b1.row2.pk.scales); swap(b1.col.pk.scales);
        swap(b1.s1.x); swap(b1.s1.y); swap(b1.s2.x); swap(b1.s2.y);
        b1.cands = b.vrow;
    } else {
        shared_scales(b1, b, true);
        b1.crange = b.r1;
        if (ps.nj == 1) b1.host_len = 1;     // (one score block: r1 = [winner, winner + 1), k_prune_pick)
    }
    if (pl.b1_bound) { b1.bound_kernel = true; b1.cache = nullptr; b1.ecache = nullptr; }
    return b1;
}
// stage A2 (second tier): the survivors `s1` of the first hull on the larger slice
Pass stage_a2_pass(const Pass& ps, const PrunePlan& pl, const PruneBufs& b, const Survivors& s1) {
    Pass a2 = slice_stage_pass(ps, pl, b.sc2, pl.k2, b.SA2);
    ranged(a2, b.r2, b.rblk2, s1);
    shared_scales(a2, b, true);
    return a2;
}
// stage B2: whatever else survives -- the hull `s` of the last tier that ran -- on all samples (an empty range when stage B1
// already covers the survivors)
Pass stage_b2_pass(const Pass& ps, const PruneBufs& b, bool second_tier, const Survivors& s) {
    Pass b2 = ps;
    ranged(b2, second_tier ? b.r3 : b.r2, second_tier ? b.rblk3 : b.rblk2, s);
    b2.scores_keep = b.S2; b2.no_select = true;
    shared_scales(b2, b, true);
    return b2;
}

// the launch records of whatever `fn` enqueues carry `stage`
template <class Fn> int run_stage(PruneStage stage, Fn&& fn) {
    g_stage = stage;
    const int rc = fn();
    g_stage = STAGE_FULL;
    return rc;
}
int launch_pick(Ctx& c, const PruneParams& pp) { return enqueue(c, KERN(PruneParams, k_prune_pick), dim3(1), dim3(256), 0, pp); }
// the hull of the survivors into pp.r_out / pp.rblk and (hm: the stream's mapped block) the named mirror slots
int launch_hull(Ctx& c, PruneParams& pp, const SelectParams& hsl, int* hm, int slot_range, int slot_blk) {
    pp.r_host = hm ? hm + slot_range : nullptr; pp.rblk_host = hm ? hm + slot_blk : nullptr;
    return enqueue(c, KERN(HullParams, k_prune_hull), dim3(1), dim3(256), 0, HullParams{pp, hsl});
}
// The survivor range a hull wrote to `r` (8 bytes), read after a stream synchronisation -- from the mirror slots where there
// is a mirror -- and, where they are mirrored (nj <= MIR_BLK), the per-block ranges.  For callers that synchronise after the
// pass anyway (pass memo): in the usual case stage B1's candidates are the only survivors (count 0) and their totals decide.
int read_survivors(Ctx& c, const int* r, const int* hm, int slot_range, int slot_blk, int nj, Survivors& s) {
    int h[2] = {0, 1};
    if (!hm) CHK(q_d2h(c, h, r, sizeof h));
    CHK(q_sync(c));
    const volatile int* m = hm;
    if (m) { h[0] = m[slot_range]; h[1] = m[slot_range + 1]; }
    s = Survivors{};
    if (h[0] >= h[1]) return 0;
    s.lo = h[0]; s.hi = h[1]; s.count = h[1] - h[0];
    if (m && nj <= MIR_BLK) { for (int i = 0; i < 2 * nj; ++i) s.blk[i] = m[slot_blk + i]; s.blk_known = true; }
    return 0;
}
// p4v_debug_bound_totals (tests): the bound's totals, the evaluated entries of stage B1's table in table order
int keep_b1_totals(Ctx& c, const float* SB, size_t n) {
    std::vector<float> h(n);
    CHK(q_d2h(c, h.data(), SB, sizeof(float) * n));
    CHK(q_sync(c));
    for (float v : h) if (v != -INFINITY) g_b1_totals.push_back(v);
    return 0;
}
// p4v_debug_prune_tables (tests): one record per staged pass, appended at the exit the pass takes.  Words of a record (include/
// ptq4vit_hip_debug.h has the same list): [0] its length, [1] 0 search pass / 1 split search, [2] round, [3] side, [4] eq_n, [5] nj,
// [6] virt, [7] hull_selects, [8] b1_bound, [9] tier 2 ran, [10] the host read the survivors, [11] the margin, [12] rows of SB's
// table (virt: 1), [13] SA2 follows, [14] S2 follows, [15] per-block ranges kept, [16..21] r1, r2, r3, [22] / [23] rows of the two
// slices; then best_idx [nj], rblk2 [2 nj], rblk3 [2 nj], SA [eq_n][nj], SB [rows][nj], SA2, S2 [eq_n][nj].  What a pass did not
// write is -1 (ranges) or absent (tables).
struct PruneKept {
    int kind, eq_n, nj; bool virt, hull_selects, b1_bound, tier2, host_read; int sb_rows, k, k2;
    const float *SA, *SB, *SA2, *S2; const int *r, *best_idx, *rblk;
};
constexpr int PRUNE_KEPT_HDR = 24;
int keep_prune_tables(Ctx& c, const PruneKept& k) {
    if (!g_tables_keep || c.dry || c.grp) return 0;
    const size_t nj = (size_t)k.nj, tab = (size_t)k.eq_n * nj, sb = (size_t)k.sb_rows * nj;
    const size_t words = PRUNE_KEPT_HDR + 5 * nj + tab + sb + (k.SA2 ? tab : 0) + (k.S2 ? tab : 0);
    std::vector<int32_t> rec(words, -1);
    const float margin = prune_margin();
    const int32_t hdr[16] = {(int32_t)words, k.kind, g_pass_round, g_pass_side, k.eq_n, k.nj, k.virt, k.hull_selects, k.b1_bound, k.tier2,
                             k.host_read, 0, k.sb_rows, k.SA2 != nullptr, k.S2 != nullptr, k.rblk != nullptr};
    std::copy(hdr, hdr + 16, rec.begin());
    std::memcpy(&rec[11], &margin, sizeof margin);
    rec[22] = k.k; rec[23] = k.k2;
    int32_t* w = rec.data() + PRUNE_KEPT_HDR;
    CHK(q_d2h(c, &rec[16], k.r, sizeof(int) * (k.tier2 ? 6 : 4)));
    if (k.virt) CHK(q_d2h(c, w, k.best_idx, sizeof(int) * nj));
    w += nj;
    if (k.rblk) CHK(q_d2h(c, w, k.rblk, sizeof(int) * (k.tier2 ? 4 : 2) * nj));
    w += 4 * nj;
    CHK(q_d2h(c, w, k.SA, sizeof(float) * tab)); w += tab;
    CHK(q_d2h(c, w, k.SB, sizeof(float) * sb)); w += sb;
    if (k.SA2) { CHK(q_d2h(c, w, k.SA2, sizeof(float) * tab)); w += tab; }
    if (k.S2) { CHK(q_d2h(c, w, k.S2, sizeof(float) * tab)); w += tab; }
    CHK(q_sync(c));
    g_tables.insert(g_tables.end(), rec.begin(), rec.end());
    return 0;
}
// nothing survives besides stage B1's candidates: the pass's selection without another sweep
int select_from_b1(Ctx& c, const Pass& ps, const PrunePlan& pl, const PruneBufs& b) {
    if (pl.hull_selects) {}          // k_prune_hull made the selection
    else if (pl.virt) {              // every block's only survivor is its stage-A winner: the table with those entries filled in
        CHK(enqueue(c, KERN(FillParams, k_fill_f32), dim3(cdiv((long)b.tab, 256)), dim3(256), 0, FillParams{b.S2, -INFINITY, (int)b.tab}));
        CHK(enqueue(c, KERN(MergeVirtParams, k_merge_virtual), dim3(cdiv(ps.nj, 64)), dim3(64), 0, MergeVirtParams{b.S2, b.SB, b.best_idx, ps.nj}));
        CHK(launch_pass_select(c, ps, b.S2));
    } else CHK(launch_pass_select(c, ps, b.SB));
    return 0;
}
int select_without_b2(Ctx& c, const Pass& ps, const PrunePlan& pl, const PruneBufs& b, const PruneKept& kept) {
    PRUNE_COUNT(PRUNE_NO_SURVIVORS);
    CHK(keep_prune_tables(c, kept));
    CHK(select_from_b1(c, ps, pl, b));
    c.ws.off = b.mark;
    return 0;
}

// plan -> buffers -> slice -> A -> pick -> B1 -> hull -> survivors -> (tier 2: slice, A2, hull, survivors) -> B2 -> merge -> select
int run_pass_pruned_impl(Ctx& c, Pass& ps) {
    PrunePlan pl;
    PruneBufs b;
    PruneOutcome outcome = plan_prune(c, ps, pl);
    if (outcome == PRUNE_STAGED) { CHK(prune_workspace(c, ps, pl, b)); CHK(fill_slice(c, ps, pl, b, outcome)); }
    if (outcome != PRUNE_STAGED) { PRUNE_COUNT(outcome); return run_pass(c, ps); }      // not eligible / keeps the full sweep
    PRUNE_COUNT(PRUNE_STAGED);
    Pass a = stage_a_pass(ps, pl, b);
    CHK(run_stage(STAGE_A, [&] { return slice_b_ok(a) ? run_slice_b(c, a, b.SA) : slice_a_ok(a) ? run_slice_a(c, a, b.SA) : run_pass(c, a); }));
    PruneParams pp{b.SA, b.SB, ps.eq_n, ps.nj, prune_margin(), b.r1, b.r1, pl.virt ? 1 : 0, b.best_idx, ps.cands, ps.cand_cs, ps.cand_js, ps.cand_off, b.vrow};
    CHK(launch_pick(c, pp));
    Pass b1 = stage_b1_pass(ps, pl, b);
    CHK(run_stage(STAGE_B1, [&] { return run_pass(c, b1); }));
    if (g_b1_keep && !c.dry && !c.grp) CHK(keep_b1_totals(c, b.SB, (size_t)b1.eq_n * ps.nj));
    // the survivors, and -- when there are none besides stage B1's candidates -- the pass's selection from its totals
    const bool host_reads = ps.host_sync_ok && !c.dry;      // the caller synchronises after this pass anyway
    int* hm = host_reads ? host_mirror(c) : nullptr;
    SelectParams hsl{b.SB, ps.eq_n, ps.nj, ps.cands, ps.cand_cs, ps.cand_js, ps.cand_off, pl.hull_selects ? ps.interval : nullptr,
                     ps.out_js, ps.out_off, ps.aux_out, ps.aux_div, nullptr, 0, ps.best_out};
    attach_mirror(hsl);
    pp.r_out = b.r2; pp.rblk = b.rblk2;
    CHK(launch_hull(c, pp, hsl, hm, MIR_R1, MIR_RB1));
    auto kept = [&](bool tier2, const float* S2) {       // p4v_debug_prune_tables: what this pass leaves at the exit it takes
        return PruneKept{0, ps.eq_n, ps.nj, pl.virt, pl.hull_selects, pl.b1_bound, tier2, host_reads, b1.eq_n, pl.k, tier2 ? pl.k2 : 0,
                         b.SA, b.SB, tier2 ? b.SA2 : nullptr, S2, b.r1, b.best_idx, b.rblk2};
    };
    Survivors s1, s2;
    if (host_reads) {
        CHK(read_survivors(c, b.r2, hm, MIR_R1, MIR_RB1, ps.nj, s1));
        if (!s1.count) return select_without_b2(c, ps, pl, b, kept(false, nullptr));     // the ~10 launches of an empty stage B2 are not made
    }
    // second tier: many survivors of a slice that holds well under all of the weight -> sweep THEM over the larger slice first
    bool second_tier = false;
    const int t2min = tune(TUNE_TIER2) >= 2 ? tune(TUNE_TIER2) : 8;
    if (b.sc2 && (c.dry || (ps.host_sync_ok && s1.count >= t2min && b.sc->frac_host < 0.9f))) {
        if (!c.dry) CHK(slice_fill(c, b.sc2, pl.geo2, /*host_sync_ok=*/false));
        Pass a2 = stage_a2_pass(ps, pl, b, s1);
        CHK(run_stage(STAGE_A2, [&] { return run_pass(c, a2); }));
        if (!c.dry) {       // same bound L* (stage B1's totals), the tighter partial sums, hull into r3
            pp.SA = b.SA2; pp.r_out = b.r3; pp.rblk = b.rblk3;
            CHK(launch_hull(c, pp, hsl, hm, MIR_R2, MIR_RB2));
            CHK(read_survivors(c, b.r3, hm, MIR_R2, MIR_RB2, ps.nj, s2));
            if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] second tier: %d survivors of the %d-row slice -> %d of the %d-row slice (M %d N %d K %d)\n", s1.count, pl.k, s2.count, pl.k2, ps.Mrows, ps.Ncols, ps.K);
            if (!s2.count) return select_without_b2(c, ps, pl, b, kept(true, nullptr));
            second_tier = true;
        }
    }
    Pass b2 = stage_b2_pass(ps, b, second_tier, second_tier ? s2 : s1);
    CHK(run_stage(STAGE_B2, [&] { return run_pass(c, b2); }));
    // Stage B2's range is the hull of ALL survivors, stage B1's candidates among them: its table decides.  The merge only fills
    // entries stage B2 did NOT evaluate (-inf) with stage B1's -- i.e. it matters when the device-side range was empty and this
    // path ran without the host knowing (no pass memo): then every block's only survivor is stage B1's candidate.
    if (!c.dry) {
        if (pl.virt) CHK(enqueue(c, KERN(MergeVirtParams, k_merge_virtual), dim3(cdiv(ps.nj, 64)), dim3(64), 0, MergeVirtParams{b.S2, b.SB, b.best_idx, ps.nj}));
        else CHK(enqueue(c, KERN(MergeParams, k_merge_scores), dim3(cdiv((long)b.tab, 256)), dim3(256), 0, MergeParams{b.S2, b.SB, (int)b.tab}));
        CHK(launch_pass_select(c, ps, b.S2));
    }
    CHK(keep_prune_tables(c, kept(second_tier, b.S2)));
    c.ws.off = b.mark;
    return 0;
}
// Variant 134217728 (debug): every eligible pruned pass is followed by the full sweep of the same pass; the selections must be
// bit-identical (the dry run plans both: the full sweep's planes live in the bump region)
int run_pass_pruned(Ctx& c, Pass& ps) {
    PrunePlan pl;
    if (!(g_variant & 134217728) || plan_prune(c, ps, pl) == PRUNE_NOT_ELIGIBLE || (!c.dry && !ps.interval)) return run_pass_pruned_impl(c, ps);
    auto full_sweep = [&] {
        Pass full = ps;
        full.prunable = false; full.scache = nullptr; full.scache2 = nullptr; full.cache = nullptr; full.ecache = nullptr;
        return run_pass(c, full);
    };
    return cross_checked(c, ps.interval, ps.out_off + (std::max(1, ps.nj) - 1) * ps.out_js + 1, "search pass",
                         [&] { return run_pass_pruned_impl(c, ps); }, full_sweep);
}

// ---- split search of the split-of-softmax matmul in one kernel (k_sos_split) -------------------------------------------------
struct SosSplitJob {
    SliceCache* scache; bool host_sync_ok, prunable;      // exact candidate pruning (run_sos_split_pruned)
    SosSplitParams kp;
    int epi; double norm;
    const float* cands; float* split; float* A_iv; float aux_div;
    float* scores_out; int scores_out_ld; int32_t* best_out;
};
bool sos_split_ok(int M, int K, int N, bool cosm) {
    return !cosm && K <= 200 && M <= 256 && N <= 64 && !(g_variant & 131072);
}
template <int KS, int VAR> int launch_sos_split_var(Ctx& c, const SosSplitParams& kp, int epi, const StatInfo* si) {
    const dim3 grid(kp.halves, kp.Z), block(256);
    const size_t lds = (size_t)2 * KS * 64 * sizeof(float);
    P4V_EPI4(epi, return enqueue(c, KERN_T(SosSplitParams, k_sos_split, KS, E, VAR), grid, block, lds, kp, si))
}
template <int KS> int launch_sos_split_ks(Ctx& c, const SosSplitParams& kp, int var, int epi, const StatInfo* si) {
    switch (var) {
        case SOS_PREV: return launch_sos_split_var<KS, SOS_PREV>(c, kp, epi, si);
        case SOS_PAIR: return launch_sos_split_var<KS, SOS_PAIR>(c, kp, epi, si);
        case SOS_LIGHT: return launch_sos_split_var<KS, SOS_LIGHT>(c, kp, epi, si);
        default: return launch_sos_split_var<KS, SOS_RES>(c, kp, epi, si);
    }
}
// The instance of k_sos_split for one sweep (see the kernel).  `known_cands`: the host's count of the candidates in `crange`, < 0
// when it does not know.  SOS_LIGHT recomputes the two images of every element per candidate, so it pays while the candidates
// are few: up to SOS_LIGHT_MAX of them (timed at ViT-B shapes with tools/sos_probe.py, docs/DESIGN_LOG.md round 13).
// Tuning 12 = 13: the previous kernel everywhere; 14: never the light instance; 15: the light instance for every known count.
constexpr int SOS_LIGHT_MAX = 2;
int sos_variant(const SosSplitParams& kp, int known_cands) {
    const int path = tune(TUNE_B1_PATH);
    if (path == 13) return SOS_PREV;
    if (kp.halves == 1 && kp.M <= 16) return SOS_PAIR;
    if (kp.halves == 1 && kp.M <= 32) return SOS_RES;           // (the unpaired share path)
    // (the light instance addresses A by 32-bit offsets from the (image, head)'s base)
    const bool a_compact = kp.a_r >= 0 && kp.a_k >= 0 && ((long)(kp.M - 1) * kp.a_r + (long)(kp.K - 1) * kp.a_k) * 4 < (1L << 31);
    if (path != 14 && a_compact && known_cands >= 1 && (known_cands <= SOS_LIGHT_MAX || path == 15)) return SOS_LIGHT;
    return SOS_RES;
}
bool sos_b_vector_ok(const SosSplitParams& kp) {
    return kp.b_n == 1 && kp.N % 4 == 0 && reinterpret_cast<uintptr_t>(kp.B) % 16 == 0 && kp.b_k % 4 == 0 && kp.b_z % 4 == 0 &&
           (kp.zdiv <= 0 || kp.b_z2 % 4 == 0);
}
// one launch of the split-search kernel on `kp` (+ k_finish into `scores`, [C] floats); `crange`: device-side candidate range
SelectParams sos_select_params(const SosSplitJob& j, const float* scores) {
    return SelectParams{scores, j.kp.C, 1, j.cands, 1, 0, 0, j.split, 0, 0, j.A_iv, j.aux_div, j.scores_out, j.scores_out_ld, j.best_out};
}
int sos_sweep(Ctx& c, SosSplitJob& j, SosSplitParams kp, const int* crange, float* scores, int known_cands = -1) {
    const int slots = kp.halves * 4;
    float* part = c.ws.get<float>((size_t)kp.C * kp.Z * slots);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    kp.part = part; kp.crange = crange;
    kp.bvec = sos_b_vector_ok(kp) ? 1 : 0;
    if (!c.dry) {
        CHK(q_fill(c, part, 0, sizeof(float) * (size_t)kp.C * kp.Z * slots));   // slots of all-padding waves
        const int KS = kp.K <= 64 ? 32 : kp.K <= 144 ? 72 : 100;
        double frac = 1.0;
        if (g_stat_on && crange && known_cands >= 0) frac = (double)known_cands / kp.C;      // (no extra round trip: see run_pass)
        else if (g_stat_on && crange) {
            int h[2] = {0, kp.C};
            CHK(q_d2h(c, h, crange, sizeof h));
            CHK(q_sync(c));
            frac = (double)std::max(0, std::min(h[1], kp.C) - std::max(h[0], 0)) / kp.C;
        }
        const StatInfo si{11, frac * (double)kp.Z * kp.halves * 128 * (2.0 * KS) * 64 * kp.C, frac * (double)kp.Z * kp.M * kp.K * kp.N * kp.C, g_stage, kp.halves, kp.Z,
                          4.0 * ((double)kp.Z * kp.M * kp.K + (double)kp.Z * kp.K * kp.N) + 8.0 * (double)kp.Z * kp.M * kp.N};
        const StatInfo* sp = &si;
        const int var = sos_variant(kp, crange ? known_cands : -1);
        if (KS == 32) CHK(launch_sos_split_ks<32>(c, kp, var, j.epi, sp));
        else if (KS == 72) CHK(launch_sos_split_ks<72>(c, kp, var, j.epi, sp));
        else CHK(launch_sos_split_ks<100>(c, kp, var, j.epi, sp));
    }
    FinishParams fp{part, (long)kp.Z * slots, (long)slots, slots, 1, kp.Z, slots, kp.C, 0, 1, 1, j.norm, scores, crange};
    return launch_finish(c, fp);
}
// p4v_debug_sos_sweep: the calling thread's next split search runs ONE sos_sweep on the first n_cands splits with the given
// candidate range and known count, and copies its [n_cands] scores out (no selection)
struct SosDebugSweep { int n_cands, c_lo, c_hi, known_cands; float* d_scores; };
thread_local const SosDebugSweep* g_sos_debug = nullptr;
int run_sos_debug_sweep(Ctx& c, SosSplitJob& j, const SosDebugSweep& dbg) {
    const size_t mark = c.ws.off;
    SosSplitParams kp = j.kp;
    kp.C = dbg.n_cands;
    float* scores = c.ws.get<float>((size_t)kp.C);
    int* r = c.ws.get<int>(2);
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    const int h[2] = {dbg.c_lo, dbg.c_hi};
    const bool ranged = dbg.c_lo >= 0;
    if (ranged) { CHK(q_h2d(c, r, h, sizeof h)); CHK(q_sync(c)); }
    CHK(sos_sweep(c, j, kp, ranged ? r : nullptr, scores, dbg.known_cands));
    HIPCHK(hipMemcpyAsync(dbg.d_scores, scores, sizeof(float) * (size_t)kp.C, hipMemcpyDeviceToDevice, c.st));
    CHK(q_sync(c));
    c.ws.off = mark;
    return 0;
}
int sos_select(Ctx& c, SosSplitJob& j, const float* scores) {
    return launch_select(c, sos_select_params(j, scores));
}
int run_sos_split(Ctx& c, SosSplitJob& j) {
    const size_t mark = c.ws.off;
    float* scores = c.ws.get<float>((size_t)j.kp.C);
    CHK(sos_sweep(c, j, j.kp, nullptr, scores));
    CHK(sos_select(c, j, scores));
    c.ws.off = mark;
    return 0;
}
// The split search with the exact pruning of run_pass_pruned: the 20 splits on the 16 heaviest query rows of every (image, head),
// the winner on everything (the bound), whatever survives on everything.  Runs once per module (its result does not depend on
// the intervals: the later rounds are memo hits), before any other pass of the module -- it is what builds the module's slice.
struct SosPruneBufs { size_t mark; float *SA, *SB, *S2; int *r1, *r2; };
// eligibility, the module's slice (allocated and filled here: this is the module's first pruned pass) and the scratch
int plan_sos_prune(Ctx& c, SosSplitJob& j, SliceGeo& geo, SosPruneBufs& b, PruneOutcome& outcome) {
    const SosSplitParams& kp = j.kp;
    outcome = (!j.prunable || !j.scache || j.scores_out || j.best_out || prune_switched_off()) ? PRUNE_NOT_ELIGIBLE
              : (kp.M < 64 || j.scache->loose) ? PRUNE_KEEP_FULL : PRUNE_STAGED;
    if (outcome != PRUNE_STAGED) return 0;
    const int k = 16;
    geo = SliceGeo{false, kp.Z, kp.M, k, kp.N, kp.K, kp.O, (kp.wt_mode == 1 ? kp.G : nullptr), kp.wt_mode, (long)kp.N, kp.A, kp.a_r, kp.a_k,
                   kp.zdiv, kp.a_z2, kp.a_z, false, PackParams{}, k};
    CHK(slice_alloc(c, j.scache, geo, true, false));
    b.mark = c.ws.off;
    b.SA = c.ws.get<float>((size_t)kp.C);
    b.SB = c.ws.get<float>((size_t)kp.C);
    b.S2 = c.ws.get<float>((size_t)kp.C);
    b.r1 = c.ws.get<int>(4);
    b.r2 = b.r1 + 2;
    if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
    if (c.dry) return 0;
    CHK(slice_fill(c, j.scache, geo, j.host_sync_ok));
    if (j.scache->loose) { c.ws.off = b.mark; outcome = PRUNE_KEEP_FULL; }
    return 0;
}
// stage A of the split search: dense slices [Z][k][K] / [Z][k][N]
SosSplitParams sos_stage_a(const SosSplitParams& kp, const SliceCache* sc, int k) {
    SosSplitParams a = kp;
    a.A = sc->Rs; a.a_k = 1; a.a_r = kp.K; a.a_z = (long)k * kp.K; a.a_z2 = (long)kp.zdiv * k * kp.K;
    a.O = sc->Os; a.G = (kp.wt_mode == 1) ? sc->Gs : sc->Os; a.M = k; a.halves = 1;
    return a;
}
// plan -> slice -> A -> pick -> B1 -> hull -> survivors -> B2 -> merge -> select: the sequence of run_pass_pruned_impl on sos_sweep
int run_sos_split_pruned_impl(Ctx& c, SosSplitJob& j) {
    const SosSplitParams& kp = j.kp;
    SliceGeo geo;
    SosPruneBufs b;
    PruneOutcome outcome;
    CHK(plan_sos_prune(c, j, geo, b, outcome));
    if (outcome != PRUNE_STAGED) { PRUNE_COUNT(outcome); return run_sos_split(c, j); }
    PRUNE_COUNT(PRUNE_STAGED);
    const SosSplitParams a = sos_stage_a(kp, j.scache, geo.k);
    CHK(run_stage(STAGE_A, [&] { return sos_sweep(c, j, a, nullptr, b.SA); }));
    PruneParams pp{b.SA, b.SB, kp.C, 1, prune_margin(), b.r1, b.r1, 0, nullptr, nullptr, 0, 0, 0, nullptr};
    CHK(launch_pick(c, pp));
    CHK(run_stage(STAGE_B1, [&] { return sos_sweep(c, j, kp, b.r1, b.SB, 1); }));      // the slice winner
    pp.r_out = b.r2;                              // (+ the selection from its totals when nothing else survives)
    if (!c.dry) {
        SelectParams hsl = sos_select_params(j, b.SB);
        attach_mirror(hsl);
        CHK(launch_hull(c, pp, hsl, nullptr, MIR_R1, MIR_RB1));
    }
    auto kept = [&](const float* S2) {               // p4v_debug_prune_tables (one score block, no per-block ranges, the hull selects)
        return PruneKept{1, kp.C, 1, false, true, false, false, j.host_sync_ok && !c.dry, kp.C, geo.k, 0, b.SA, b.SB, nullptr, S2, b.r1, nullptr, nullptr};
    };
    int survivors = -1;
    if (j.host_sync_ok && !c.dry) {
        Survivors s;
        CHK(read_survivors(c, b.r2, nullptr, MIR_R1, MIR_RB1, 1, s));
        if (!s.count) { PRUNE_COUNT(PRUNE_NO_SURVIVORS); CHK(keep_prune_tables(c, kept(nullptr))); c.ws.off = b.mark; return 0; }
        survivors = std::max(0, std::min(s.hi, kp.C) - std::max(s.lo, 0));
    }
    CHK(run_stage(STAGE_B2, [&] { return sos_sweep(c, j, kp, b.r2, b.S2, survivors); }));
    if (!c.dry) CHK(enqueue(c, KERN(MergeParams, k_merge_scores), dim3(1), dim3(256), 0, MergeParams{b.S2, b.SB, kp.C}));
    CHK(sos_select(c, j, b.S2));
    CHK(keep_prune_tables(c, kept(b.S2)));
    c.ws.off = b.mark;
    return 0;
}
// (the cross-check of run_pass_pruned; the dry run plans the pruned search only: same scratch)
int run_sos_split_pruned(Ctx& c, SosSplitJob& j) {
    if (!(g_variant & 134217728) || c.dry || !j.split) return run_sos_split_pruned_impl(c, j);
    return cross_checked(c, j.split, 1, "split search", [&] { return run_sos_split_pruned_impl(c, j); }, [&] { return run_sos_split(c, j); });
}

// ---- exact memoisation of search passes ---------------------------------------------------------------------
// Every candidate table is built once from the initial interval (reference linear.py:544-545), so a search pass
// is a deterministic function of the counterpart's CURRENT interval only.  Rounds 2-3 often see an interval that
// was already evaluated (the alternation has converged): the pass would recompute, bit for bit, the selection it
// produced before.  Such a pass is skipped and its recorded output restored.  Exact by construction (the kernels
// are deterministic); disabled when the caller asks for score tables, or with desc.reserved bit 1.
struct PassMemo {
    struct Entry { std::vector<float> in, out; };
    std::vector<Entry> entries;
    const std::vector<float>* find(const std::vector<float>& in) const {
        for (const auto& e : entries)
            if (e.in.size() == in.size() && std::memcmp(e.in.data(), in.data(), in.size() * sizeof(float)) == 0) return &e.out;
        return nullptr;
    }
};

int read_dev(Ctx& c, const float* d, int n, std::vector<float>& h) {
    h.resize(n);
    if (IvMirror* m = mirror_of(d); m && m->valid && m->count == n) {      // the selection that wrote `d` also wrote the mirror
        CHK(q_sync(c));
        const volatile float* src = m->host;
        for (int i = 0; i < n; ++i) h[i] = src[i];
        return 0;
    }
    CHK(q_d2h(c, h.data(), d, sizeof(float) * n));
    return q_sync(c);
}

int write_dev(Ctx& c, float* d, const std::vector<float>& h) {
    if (IvMirror* m = mirror_of(d)) m->valid = false;
    CHK(q_h2d(c, d, h.data(), sizeof(float) * h.size()));
    if (c.grp) return 0;                    // (a group's queue holds a copy of the data: the restore needs no round trip)
    return q_sync(c);                       // h may go out of scope
}

// Up to two device vectors: the key or the value of one side's memo.  None: a pass that depends on nothing.
struct DevVecs {
    int count; float* d[2]; int n[2];
    DevVecs(float* d0 = nullptr, int n0 = 0, float* d1 = nullptr, int n1 = 0) : count(n1 ? 2 : n0 ? 1 : 0), d{d0, d1}, n{n0, n1} {}
};
// read one after the other (each read_dev is a rendezvous), concatenated
int read_vecs(Ctx& c, const DevVecs& vs, std::vector<float>& h) {
    std::vector<float> part;
    h.clear();
    for (int i = 0; i < vs.count; ++i) { CHK(read_dev(c, vs.d[i], vs.n[i], part)); h.insert(h.end(), part.begin(), part.end()); }
    return 0;
}
// A host copy of an interval vector, valid while no pass has moved the vector since (Linear: what a pass just read back or
// restored is the next pass's key -- no second read-back)
struct HostCopy { std::vector<float> v; bool ok = false; };

// The pass memo of ONE side of a module's alternating search: restore() before the side's passes, record() after them when
// restore() reported no hit.  Switched off (`on` false) both do nothing but invalidate the caller's host copy of the value.
struct MemoSide {
    bool on = false;
    PassMemo table;
    std::vector<float> key;      // of the lookup in flight: record() files the value under it
    // key: `key_host` when the caller holds a valid copy, else the key vectors read back; no vectors: the constant key {0}.
    // On a hit the recorded value goes back into `out` (write_dev: no synchronisation inside a group).
    int restore(Ctx& c, const DevVecs& key_vecs, const HostCopy* key_host, const DevVecs& out, HostCopy* out_host, bool* hit) {
        *hit = false;
        if (!on) return 0;
        if (key_host && key_host->ok) key = key_host->v;
        else if (key_vecs.count == 0) key.assign(1, 0.0f);
        else CHK(read_vecs(c, key_vecs, key));
        const std::vector<float>* val = table.find(key);
        if (!val) return 0;
        size_t off = 0;
        for (int i = 0; i < out.count; off += out.n[i], ++i)
            CHK(write_dev(c, out.d[i], std::vector<float>(val->begin() + off, val->begin() + off + out.n[i])));
        g_memo_hits++;
        if (out_host) { out_host->v = *val; out_host->ok = true; }
        *hit = true;
        return 0;
    }
    int record(Ctx& c, const DevVecs& out, HostCopy* out_host) {
        if (!on) { if (out_host) out_host->ok = false; return 0; }     // the passes moved `out`, nobody read it back
        std::vector<float> val;
        CHK(read_vecs(c, out, val));
        table.entries.push_back({key, val});
        g_memo_misses++;
        if (out_host) { out_host->v = val; out_host->ok = true; }
        return 0;
    }
};

// binds the interval vectors of one *_impl call (the ones its pass memo reads back) to the stream's mapped block
struct MirrorScope {
    MirrorScope(Ctx& c, bool on, const float* a, const float* b = nullptr, const float* d3 = nullptr) {
        float* base = (on && !c.dry) ? reinterpret_cast<float*>(host_mirror(c)) : nullptr;
        const float* devs[MIR_SLOTS] = {a, b, d3};
        for (int i = 0; i < MIR_SLOTS; ++i)
            g_mir[i] = IvMirror{(base && devs[i]) ? devs[i] : nullptr, base ? base + MIR_HDR + i * MIR_SLOT : nullptr, false, 0};
    }
    ~MirrorScope() { for (auto& m : g_mir) m = IvMirror{}; }
    MirrorScope(const MirrorScope&) = delete;
    MirrorScope& operator=(const MirrorScope&) = delete;
};

// The mode of one *_impl call.  The fused entry points run all of calibration_step2 (ST_ALL: initialisation, then
// search_round x {first operand, second operand} with memoisation); the granular entry points of the C ABI
// (p4v_amax_init_*, p4v_*_search_*) run ONE part with the candidate table supplied by the caller, the way the reference's
// _initialize_intervals / _search_best_*_interval methods are called one by one (linear.py:380-397,455-533); ST_FWD is
// quant_forward: the intervals are INPUTS, nothing is initialised or searched.  A sizing run (Ctx::dry) has the mode of the
// call it sizes; what a mode reads of the call's tensor record is checked for presence in real calls only.
enum { ST_INIT = 1, ST_S1 = 2, ST_S2 = 4, ST_ALL = 7, ST_FWD = 8 };
struct Stage {
    int mask = ST_ALL;
    const float* cands1 = nullptr;   // caller's candidate table of the first operand  (w / A), used when ST_INIT is not set
    const float* cands2 = nullptr;   // ... of the second operand (a / B)
    bool full() const { return mask == ST_ALL; }
    bool searches() const { return (mask & (ST_S1 | ST_S2)) != 0; }
    bool forward() const { return mask == ST_FWD; }
    bool inits() const { return (mask & ST_INIT) != 0; }
};

// Bits of a descriptor's `reserved` word (include/ptq4vit_hip.h documents which descriptor reads which): the generic fp32-operand
// path of a Linear, no pass memo, *_workspace_bytes sizes for *_quant_forward alone (the sizing run's mode is ST_FWD), no exact
// candidate pruning; bits 8..11 (p4v_linear_search_w / _a): 1 + b runs the step of block b alone; -1: every block in turn
enum : int { RSV_FP32_PLANES = 1, RSV_NO_MEMO = 2, RSV_FORWARD_ONLY = 4, RSV_NO_PRUNE = 8 };
inline int reserved_block(int reserved) { return ((reserved >> 8) & 15) - 1; }
inline Stage sizing_stage(int reserved) { return (reserved & RSV_FORWARD_ONLY) ? Stage{ST_FWD} : Stage{}; }

// What the round loop of a *_impl call derives from its Stage, its descriptor and the caller's tables.
struct SearchRounds {
    bool memo_on = false;        // the pass memo: a fused call that really runs, returns no tables and has not switched it off
    bool keep_planes = false;    // candidate-expanded planes stay packed between the rounds of a fused call
    int n_rounds = 1;            // a granular call is one pass
    bool full = true;            // fused call: slot [round][which] of the tables; granular call: the one table of the call
    int per_round = 2;           // tables per round: the two sides (MatMul with sub-blocks: one per block step)
    int eq_n = 0, ld = 0;        // a score table is [eq_n][ld], a selection [ld]
    float* scores = nullptr;
    int32_t* best = nullptr;
    SearchRounds() {}
    SearchRounds(const Stage& sg, int search_round, bool memo_allowed, int eq_n_, int ld_, const Ctx& c, float* scores_out, int32_t* best_out,
                 int per_round_ = 2)
        : memo_on(sg.full() && !c.dry && !scores_out && !best_out && memo_allowed), keep_planes(sg.full() && search_round > 1),
          n_rounds(sg.full() ? search_round : 1), full(sg.full()), per_round(per_round_), eq_n(eq_n_), ld(ld_), scores(scores_out),
          best(best_out) {}
    long slot(int round, int which) const { return full ? (long)round * per_round + which : 0; }
    float* scores_of(int round, int which) const { return scores ? scores + slot(round, which) * eq_n * ld : nullptr; }
    int32_t* best_of(int round, int which) const { return best ? best + slot(round, which) * ld : nullptr; }
};

// One side of a module's alternating search: its Stage bit (0: the call has no such side), its pass memo, the device vectors the
// memo keys on and the ones it restores / records, and run(round), which builds and runs the side's passes of one round.
struct SearchSide {
    int bit;
    MemoSide memo;
    DevVecs key, val;
    std::function<int(int)> run;
    SearchSide(int bit_, bool memo_on, const DevVecs& key_, const DevVecs& val_, std::function<int(int)> run_)
        : bit(bit_), key(key_), val(val_), run(std::move(run_)) { memo.on = memo_on; }
};
// The alternation of Linear, MatMul and Conv: for round, for side: restore the memo, run the side's passes unless it hit, record.
// `host` (Linear; null: the key is read back): host copies of the two values, host[1 - s] the key of side s.
// The form is "record whenever the restore did not hit", whether or not the call's mask has the side's bit.  That is also "record
// only after the passes ran", the form the MatMul B side and both Conv sides had: a memo that is on implies Stage::full()
// (SearchRounds::memo_on), so every side that has a memo switched on has its bit in the mask, and the mask test and the record
// commute; with the memo off record() only invalidates the caller's host copy -- nothing without `host`, and with it what Linear
// always did for a side that may have moved its value.  For the same reason it does not matter whether the mask is tested
// before or after restore(): with the memo off restore() does nothing.  A side with bit 0 (Conv's activations with a_bit >= 32)
// has its memo off and never runs.  A run() that ends a granular call early with 0 (p4v_debug_sos_sweep) is the call's only pass.
int search_rounds(Ctx& c, const SearchRounds& R, const Stage& sg, SearchSide (&sides)[2], HostCopy* host) {
    for (int round = 0; round < R.n_rounds; ++round)
        for (int s = 0; s < 2; ++s) {
            SearchSide& sd = sides[s];
            bool hit = false;
            CHK(sd.memo.restore(c, sd.key, host ? &host[1 - s] : nullptr, sd.val, host ? &host[s] : nullptr, &hit));
            if (hit) continue;
            g_pass_round = round; g_pass_side = s;
            const int rc_run = (sg.mask & sd.bit) ? sd.run(round) : 0;
            g_pass_round = g_pass_side = -1;
            CHK(rc_run);
            CHK(sd.memo.record(c, sd.val, host ? &host[s] : nullptr));
        }
    return 0;
}

PackParams pack2d(const float* src, long rows, long cols, long ld) {
    PackParams p{};
    p.src = src; p.s_z = 0; p.s_r = ld; p.s_k = 1; p.Z = 1; p.R = (int)rows; p.K = (int)cols;
    p.mode = PACK_SYM; p.nblk_r = 1; p.nblk_k = 1;
    return p;
}

// The K-segment table of a SegPlan whose sizes and block counts are set: K cut at every multiple of A's column-block width and
// of B's row-block width, S <= n_H_A + n_V_B - 1 segments
int seg_cut_k(SegPlan& g, const char* who) {
    const int K = g.K;
    if (K >= 16384) return fail(P4V_ERR_UNSUPPORTED, "%s: K < 16384 with sub-blocks", who);
    std::vector<int> cuts{0};
    for (int i = 1; i < g.nHA; ++i) if (i * g.ccA < K) cuts.push_back(i * g.ccA);
    for (int i = 1; i < g.nVB; ++i) if (i * g.crB < K) cuts.push_back(i * g.crB);
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    if ((int)cuts.size() > SEG_MAX - 1) return fail(P4V_ERR_UNSUPPORTED, "%s: more than %d K segments", who, SEG_MAX - 1);
    g.seg.S = (int)cuts.size();
    int dpos = 0;
    for (int s = 0; s < g.seg.S; ++s) {
        const int k1 = s + 1 < g.seg.S ? cuts[s + 1] : K;
        g.seg.k0[s] = (short)cuts[s]; g.seg.d0[s] = (short)dpos;
        g.ablk[s] = (unsigned char)(cuts[s] / g.ccA); g.bblk[s] = (unsigned char)(cuts[s] / g.crB);
        dpos += (int)rup(k1 - cuts[s], 64);
    }
    for (int s = g.seg.S; s <= SEG_MAX; ++s) { g.seg.k0[s] = (short)K; g.seg.d0[s] = (short)dpos; }
    g.Kseg = dpos;
    if (g.Kseg / SW_BKB > SEG_KT_MAX) return fail(P4V_ERR_UNSUPPORTED, "%s: K too large for the segment table", who);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Linear
// ------------------------------------------------------------------------------------------------
// The device pointers of one linear_impl call, filled by name at the entry points; what the call's mode (Stage) does not read
// stays null, and a sizing run leaves all of them null.
struct LinearTensors {
    const float *W = nullptr, *bias = nullptr, *X = nullptr;    // weight [N][K], bias [N] (null: none), x [M][K]
    const float *O = nullptr, *G = nullptr;                     // raw_out / raw_grad [M][N] (searches; G: the hessian metric)
    const float* mult = nullptr;                                // [eq_n + 1] candidate multipliers (ST_INIT with a search)
    float *w_iv = nullptr, *a_iv = nullptr;                     // intervals [n_V][n_H] / [n_a]: out, in / out, or -- ST_FWD -- in
    float* scores = nullptr; int32_t* best = nullptr;           // optional score tables / selections
    float* fwd_out = nullptr;                                   // ST_FWD: the destination [M][N]
};
// One linear_impl call: what build() derives from the descriptor, and the builders of its passes.  Sides: 0 = the weight search
// (reference linear.py:455-495), 1 = the activation search (linear.py:497-533 / 609-642).
struct LinearCall {
    Ctx& c;
    const p4v_linear_desc* d;
    const LinearTensors t;
    const Stage& sg;
    int M = 0, K = 0, N = 0;                          // samples (batch x tokens), in_features, out_features
    int nV = 1, nH = 1, nA = 1;                       // row / column blocks of the weights, column blocks of the activations
    int crb_rows = 0, crb_cols = 0, crb_acts = 0;     // ... and their sizes
    int wq = 0, aq = 0;                               // 2^(bit - 1) of the weights / the activations
    float a_neg = 0.f;                                // the fixed scale of the post-GELU negative range (linear.py:574)
    int epi = 0, wt_mode = 0;                         // the metric's epilogue and weighting (metric_epi)
    int ncand = 0;                                    // rows of a candidate table: eq_n + 1
    bool cosm = false;                                // cosine metric
    bool general = false;                             // fp32 candidate planes: column / activation blocks, desc.reserved bit 0, cosine on the twin
    bool i8 = false;                                  // int8 planes (everything else)
    bool twin = false;                                // post-GELU on int8 planes: the activations as two planes (positive / negative range)
    bool segcos = false;                              // cosine with column / activation blocks: the K-segmented int8 sweep, one block step per pass
    bool cos6 = false, cos7 = false;                  // cosine in the orientation of the difference metrics, on k_sweep6 / k_sweep7
    int only_blk = -1;                                // granular call, desc.reserved bits 8..11 = 1 + b: the step of block b alone; else -1
    int tab_blk = 0;                                  // the block whose score table and selections the call returns
    unsigned *enc_w = nullptr, *enc_a = nullptr;      // abs-max per block, order-preserving encoding
    float *w_cands_ws = nullptr, *a_cands_ws = nullptr;       // candidate tables built by this call ...
    const float *w_cands = nullptr, *a_cands = nullptr;       // ... or the caller's (granular search)
    float* Ufold = nullptr;                           // twin activation search: the target with the negative plane folded in
    float *w_mix = nullptr, *a_mix = nullptr;         // general path: candidates in the searched block's column, the current interval elsewhere
    float* Ot = nullptr;                              // segcos: raw_out as [feature][sample] (the seg sweep's rows are features)
    SegPlan sgp{};                                    // segcos: A := W as n_V heads, B := x shared by the heads
    SearchRounds rounds;
    PlaneCache plane[2];                              // per side: the candidate-expanded plane, kept across rounds
    EpiCache ecache[2];                               // per side: k_sweep6's epilogue operands in fragment order
    SliceCache slice, slice2;                         // the sample slices of the pruned passes (two tiers)

    LinearCall(Ctx& c_, const p4v_linear_desc* d_, const LinearTensors& t_, const Stage& sg_) : c(c_), d(d_), t(grad_by_metric(t_, d_->metric)), sg(sg_) {}

    // argument checks, geometry, the path decisions, the workspace
    int build() {
        M = d->batch * d->tokens; K = d->in_features; N = d->out_features;
        nV = d->n_V; nH = d->n_H; nA = d->n_a;
        if (M <= 0 || K <= 0 || N <= 0 || nV <= 0 || nH <= 0 || nA <= 0 || d->eq_n <= 0)
            return fail(P4V_ERR_INVALID, "linear: non-positive dimension");
        if (N % nV || K % nH || K % nA) return fail(P4V_ERR_UNSUPPORTED, "linear: n_V/n_H/n_a must divide the layer (reference ignores remainders, linear.py:118)");
        if (d->w_bit > 8 || d->a_bit > 8 || d->w_bit < 2 || d->a_bit < 2) return fail(P4V_ERR_UNSUPPORTED, "linear: bit widths 2..8 supported");
        crb_rows = N / nV; crb_cols = K / nH; crb_acts = K / nA;
        wq = 1 << (d->w_bit - 1); aq = 1 << (d->a_bit - 1);
        a_neg = (float)(0.16997124254703522 / aq);   // linear.py:574
        metric_epi(d->metric, &epi, &wt_mode);
        cosm = epi == EPI_COS;
        if (wt_mode == 1 && !t.G && sg.searches() && !c.dry) return fail(P4V_ERR_INVALID, "linear: hessian metric needs raw_grad (linear.py:418)");
        general = (nH > 1 || nA > 1 || (d->reserved & RSV_FP32_PLANES) || (cosm && d->twin_postgelu && !sg.forward()));
        i8 = !general;
        twin = d->twin_postgelu && i8;
        // Cosine with column / activation blocks (linear.py:455-533): the K-segmented int8 sweep, transposed -- A := W as n_V heads of
        // crb_rows x K with intervals w_iv[v][h], B := x as K x samples shared by the heads with intervals a_iv[a]; K cut at the
        // multiples of crb_cols and crb_acts.  One block step per pass (run_pass_seg), every other block on the interval entering it.
        segcos = cosm && !sg.forward() && (nH > 1 || nA > 1);
        if (segcos && d->twin_postgelu)
            return fail(P4V_ERR_UNSUPPORTED, "linear: cosine with n_H>1 / n_a>1 on the post-GELU twin is not implemented on the GPU "
                                             "(the twin's second plane lies on the column side, k_sweep_seg has no instance for that)");
        if (segcos) {
            if (nH > 8 || nA > 8) return fail(P4V_ERR_UNSUPPORTED, "linear: cosine with up to n_H, n_a = 8 blocks is implemented on the GPU");
            sgp.batch = 1; sgp.H = nV; sgp.M = crb_rows; sgp.K = K; sgp.N = M;
            sgp.nVA = 1; sgp.nHA = nH; sgp.nVB = nA; sgp.nHB = 1;
            sgp.crA = crb_rows; sgp.ccA = crb_cols; sgp.crB = crb_acts; sgp.ccB = M;
            sgp.A = t.W; sgp.a_st[0] = 0; sgp.a_st[1] = (long)crb_rows * K; sgp.a_st[2] = K; sgp.a_st[3] = 1;
            sgp.B = t.X; sgp.b_st[0] = 0; sgp.b_st[1] = 0; sgp.b_st[2] = 1; sgp.b_st[3] = K; sgp.b_shared = true;
            sgp.Aq = wq; sgp.Bq = aq; sgp.ivA = t.w_iv; sgp.ivB = t.a_iv;
            CHK(seg_cut_k(sgp, "linear"));
        }
        rounds = SearchRounds(sg, d->search_round, !(d->reserved & RSV_NO_MEMO), d->eq_n, nV, c, t.scores, t.best);
        only_blk = sg.full() ? -1 : reserved_block(d->reserved);
        if (sg.searches() && only_blk >= ((sg.mask & ST_S1) ? nH : nA)) return fail(P4V_ERR_INVALID, "linear: block %d outside the layer's blocks", only_blk);
        tab_blk = std::max(0, only_blk);
        // Cosine on k_sweep6: the layer as ONE GEMM in the orientation of the difference metrics (rows = samples, columns =
        // features), the register-stationary sweep with the cosine epilogues EPI_COS / EPI_COS_T; the V blocks are runs of 64-feature
        // slabs of k_finish_cos's table.  Otherwise (K > 768, blocks that are not whole slabs, variant 2048): k_sweep2 on the swapped
        // operands, one GEMM per V block.
        cos6 = cosm && i8 && !twin && !general && nH == 1 && nA == 1 && (nV == 1 || crb_rows % 64 == 0) &&
               sweep6_supported((int)(rup(K, 64) / 64)) && !(g_variant & (4 | 2048)) && !g_force_v1;
        // ... and on k_sweep7 for K >= 1024 (fc2): 128-feature slabs; the conditions are run_pass's for that kernel
        cos7 = cosm && i8 && !twin && !general && nH == 1 && nA == 1 && (nV == 1 || crb_rows % 128 == 0) && !cos6 &&
               rup(K, 64) >= 1024 && rup(K, 64) % 256 == 0 && N % 32 == 0 && (long)M * N * 4 < (1L << 32) &&
               (c.dry || (((unsigned long long)t.O) & 15) == 0) && !(g_variant & (2048 | 32768)) && !g_force_v1;
        ncand = d->eq_n + 1;
        cvt_bias(c);     // (first call of the process: probe the conversion quant16_sat8 relies on)
        enc_w = c.ws.get<unsigned>((size_t)nV * nH);
        enc_a = c.ws.get<unsigned>((size_t)nA);
        w_cands_ws = c.ws.get<float>((size_t)ncand * nV * nH);
        a_cands_ws = c.ws.get<float>((size_t)ncand * nA);
        w_cands = sg.inits() ? w_cands_ws : sg.cands1;
        a_cands = sg.inits() ? a_cands_ws : sg.cands2;
        Ufold = twin ? c.ws.get<float>((size_t)M * N) : nullptr;
        w_mix = c.ws.get<float>((size_t)ncand * nV * nH);
        a_mix = c.ws.get<float>((size_t)ncand * nA);
        Ot = segcos ? c.ws.get<float>((size_t)M * N) : nullptr;
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small");
        return 0;
    }

    // interval initialisation of one side (linear.py:380-397 / 576-599): abs-max per block, the interval, its candidate table
    int init_side(int side) {
        if (!sg.inits()) return 0;
        const long stw[4] = {0, 0, K, 1};
        if (side == 0) {
            CHK(launch_absmax(c, t.W, stw, 1, 1, N, K, nV, nH, crb_rows, crb_cols, 0, enc_w));
            CHK(launch_interval(c, enc_w, nV * nH, (float)(wq - 0.5), d->init_layerwise, t.w_iv));
            if (sg.searches()) CHK(launch_cands(c, t.mult, t.w_iv, ncand, nV * nH, w_cands_ws));
        } else {
            CHK(launch_absmax(c, t.X, stw, 1, 1, M, K, 1, nA, M, crb_acts, d->twin_postgelu ? 1 : 0, enc_a));
            CHK(launch_interval(c, enc_a, nA, (float)(aq - 0.5), d->init_layerwise, t.a_iv));
            if (sg.searches()) CHK(launch_cands(c, t.mult, t.a_iv, ncand, nA, a_cands_ws));
        }
        return 0;
    }

    Operand x_operand(bool expanded, const float* scales, int sc_cs) const {
        Operand op{};
        op.present = true; op.expanded = expanded;
        op.pk = pack2d(t.X, M, K, K);
        op.pk.scales = scales; op.pk.sc_cs = sc_cs;
        op.pk.lo = -aq; op.pk.hi = aq - 1;
        if (nA > 1) { op.pk.blk_mode = 1; op.pk.blk_div = INT_MAX; op.pk.nblk_r = 1; op.pk.nblk_k = nA; op.pk.blk_div2 = crb_acts; }
        if (d->twin_postgelu) {
            if (i8) { op.pk.lo = 0; }
            else { op.pk.mode = PACK_TWIN_SIM; op.pk.lo = -aq; op.pk.neg_scale = a_neg; }
        }
        return op;
    }
    Operand xneg_operand() const {
        Operand op{};
        op.present = true; op.expanded = false;
        op.pk = pack2d(t.X, M, K, K);
        op.pk.scales = nullptr; op.pk.neg_scale = a_neg; op.pk.lo = -aq; op.pk.hi = 0;
        return op;
    }
    Operand w_operand(bool expanded, const float* scales, int sc_cs, bool by_vblock) const {
        Operand op{};
        op.present = true; op.expanded = expanded;
        if (by_vblock) {   // swapped cosine sweep: one GEMM per V block
            op.pk = pack2d(t.W, crb_rows, K, K);
            op.pk.s_z = (long)crb_rows * K;
            op.pk.blk_mode = 2; op.pk.blk_div = nV;
            if (nH > 1) return op;  // unreachable: general path is not swapped per block
        } else {
            op.pk = pack2d(t.W, N, K, K);
            op.pk.blk_mode = 1; op.pk.blk_div = crb_rows; op.pk.nblk_r = nV; op.pk.nblk_k = nH;
            op.pk.blk_div2 = nH > 1 ? crb_cols : 0;
        }
        op.pk.scales = scales; op.pk.sc_cs = sc_cs;
        op.pk.lo = -wq; op.pk.hi = wq - 1;
        return op;
    }

    // out = Q_a(x) . Q_w(W)^T + bias as ONE integer GEMM: grid indices packed to int8 planes (the twin's two ranges
    // as two planes), scales s_a * s_w[block] applied to the int32 accumulators in the epilogue
    Pass forward_pass() const {
        Pass fp{};
        fp.i8 = i8; fp.twin = twin; fp.epi = EPI_FWD; fp.wt_mode = 0; fp.eq_n = 1; fp.K = K;
        fp.Z = 1; fp.Mrows = M; fp.Ncols = N;
        fp.row = x_operand(false, t.a_iv, 0);
        if (twin) fp.row2 = xneg_operand();
        fp.col = w_operand(false, t.w_iv, 0, false);
        fp.use_s1 = i8; fp.s_cs = nV; fp.sb_mode = 1; fp.sb_div = crb_rows;
        fp.s1 = ScaleParams{t.a_iv, 0, 0, 0.f, t.w_iv, 0, 1, 0.f, 0, 0, nullptr};
        fp.s2 = ScaleParams{nullptr, 0, 0, a_neg, t.w_iv, 0, 1, 0.f, 0, 0, nullptr};
        fp.bias = t.bias; fp.bias_axis = 0; fp.bias_zs = 0;
        fp.O = t.fwd_out; fp.G = nullptr; fp.o_ms = N; fp.o_ns = 1; fp.o_inner = INT_MAX;
        fp.nj = 1; fp.store_out = t.fwd_out;
        return fp;
    }

    // what a pass of (side, round, block) selects from and writes: one score per V block (weights) or one for the layer, the
    // block's column of the side's candidate table and of its intervals; tables of the first block only (granular: of the one asked for)
    void selection(Pass& ps, int side, int round, int blk) const {
        const bool ws = side == 0;
        ps.nj = ws ? nV : 1; ps.cands = ws ? w_cands : a_cands; ps.cand_cs = ws ? nV * nH : nA; ps.cand_js = ws ? nH : 0; ps.cand_off = blk;
        ps.interval = ws ? t.w_iv : t.a_iv; ps.out_js = ws ? nH : 0; ps.out_off = blk;
        if (blk == tab_blk) { ps.scores_out = rounds.scores_of(round, side); ps.best_out = rounds.best_of(round, side); }
        ps.scores_out_ld = nV;
    }
    // The search pass of (side, round, block).  The side chooses the expanded operand and its table `cands` ([ncand][cs]: the
    // side's candidate table, or its mix), what s1 reads, one score per V block or one for the layer; the orientation is the metric's.
    Pass search_pass(int side, int round, int blk, const float* cands, bool host_sync_ok) {
        const bool ws = side == 0;
        const int cs = ws ? nV * nH : nA;
        Pass ps{};
        ps.i8 = i8; ps.twin = twin; ps.epi = epi; ps.wt_mode = wt_mode; ps.eq_n = d->eq_n; ps.K = K;
        ps.cache = (rounds.keep_planes && (ws ? nH : nA) == 1) ? &plane[side] : nullptr;   // (blocks: the table mixes in the current interval)
        ps.ecache = rounds.keep_planes ? &ecache[side] : nullptr;
        selection(ps, side, round, blk);
        const bool dense = !cosm || cos6 || cos7;
        const Operand xo = ws ? x_operand(false, t.a_iv, 0) : x_operand(true, cands, cs);
        const Operand wo = ws ? w_operand(true, cands, cs, !dense) : w_operand(false, t.w_iv, 0, !dense);
        ps.s1 = ws ? ScaleParams{t.a_iv, 0, 0, 0.f, w_cands, nV, 1, 0.f, 0, 0, nullptr} : ScaleParams{a_cands, 1, 0, 0.f, t.w_iv, 0, 1, 0.f, 0, 0, nullptr};
        ps.use_s1 = i8; ps.s_cs = nV;
        ps.bias = t.bias; ps.O = t.O; ps.o_inner = INT_MAX;
        if (dense) {
            // rows = samples, columns = features
            ps.Z = 1; ps.Mrows = M; ps.Ncols = N;
            ps.row = xo; ps.col = wo;
            if (twin) { ps.row2 = xneg_operand(); ps.twin_disjoint = ws; }    // linear.py:605-606: clamp(.,0,q-1) / clamp(.,-q,0)
            ps.sb_mode = 1; ps.sb_div = crb_rows;
            ps.s2 = ScaleParams{nullptr, 0, 0, a_neg, ws ? w_cands : t.w_iv, ws ? nV : 0, 1, 0.f, 0, 0, nullptr};
            ps.bias_axis = 0; ps.bias_zs = 0;
            ps.G = t.G; ps.o_zs = 0; ps.o_bs = 0; ps.o_ms = N; ps.o_ns = 1;
            ps.j_mode = ws ? 1 : 0; ps.j_div = ws ? crb_rows : 0;
            ps.norm = 1.0 / ((double)d->tokens * (ws ? crb_rows : N));
            ps.prunable = !(d->reserved & RSV_NO_PRUNE); ps.scache = &slice; ps.scache2 = &slice2; ps.host_sync_ok = host_sync_ok;
            if (cos6 || cos7) {
                ps.cos6 = cos6; ps.cos7 = cos7; ps.G = nullptr; ps.wt_mode = 0; ps.prunable = false; ps.scache = nullptr; ps.scache2 = nullptr;
                ps.cos_ZB = 1; ps.cos_ZV = nV; ps.cos_j_mode = ws ? 1 : 0;
                ps.norm = 1.0 / (double)d->tokens;
            }
        } else {
            // swapped: rows = features of V block z, columns = samples -- one GEMM per V block
            ps.Z = nV; ps.Mrows = crb_rows; ps.Ncols = M;
            ps.row = wo; ps.col = xo;
            ps.col_zs_shared = 1;
            ps.sb_mode = 2; ps.sb_div = nV;
            ps.bias_axis = 1; ps.bias_zs = crb_rows;
            ps.G = nullptr; ps.o_zs = crb_rows; ps.o_bs = 0; ps.o_ms = 1; ps.o_ns = N;
            ps.cos_ZB = 1; ps.cos_ZV = nV; ps.cos_j_mode = ws ? 1 : 0;
            ps.norm = 1.0 / (double)d->tokens;
        }
        return ps;
    }

    // the block step of the cosine seg sweep: side 0 = column block h of every V block (one score per V block), side 1 =
    // activation block a (ONE score over all features); tables of block 0 only, as for the difference metrics
    Pass seg_cos_pass(int side, int round, int blk) {
        const bool ws = side == 0;
        sgp.side = side + 1; sgp.ov_v = ws ? 0 : blk; sgp.ov_h = ws ? blk : 0;
        sgp.cands = (ws ? w_cands : a_cands) + blk; sgp.cand_cs = ws ? nV * nH : nA; sgp.cand_hs = ws ? nH : 0;
        Pass ps{};
        ps.seg = &sgp; ps.i8 = true; ps.epi = EPI_COS; ps.eq_n = d->eq_n; ps.K = K;
        ps.Z = nV; ps.Mrows = crb_rows; ps.Ncols = M;
        ps.bias = t.bias; ps.bias_axis = 1; ps.bias_zs = crb_rows;
        ps.O = Ot;
        ps.cos_ZB = 1; ps.cos_ZV = nV; ps.cos_j_mode = ws ? 1 : 0;
        ps.norm = 1.0 / (double)d->tokens;
        selection(ps, side, round, blk);
        return ps;
    }

    // General path with blocks: the candidates replace block `blk` only, the others keep the current interval (linear.py:468-469):
    // mix[c][j] = (j in block blk) ? cands[c][j] : interval[j] -- a broadcast of the interval, then the block's column(s) copied in
    int mix_candidates(int side, int blk) {
        if (c.dry) return 0;
        const bool ws = side == 0;
        const int n = ws ? nV * nH : nA, rows = ws ? nV : 1;
        const float* cands = ws ? w_cands : a_cands;
        float* mix = ws ? w_mix : a_mix;
        ScaleParams mp{};
        mp.x = ws ? t.w_iv : t.a_iv; mp.x_cs = 0; mp.x_js = 1; mp.y = nullptr; mp.y_const = 1.0f; mp.C = ncand; mp.nblk = n; mp.S = mix;
        mp.copy = 1;                      // (the fp32 packers divide by these themselves: a zero interval stays 0, its plane is 0 / 0)
        CHK(launch_scale(c, mp));
        for (int v = 0; v < rows; ++v)
            CHK(q_copy2d(c, mix + v * nH + blk, sizeof(float) * n, cands + v * nH + blk, sizeof(float) * n, sizeof(float), ncand));
        return 0;
    }

    // Twin activation search: the negative-range plane and the weights are candidate-invariant, so their product is folded
    // into the target once (U = raw_out - bias - s_neg*s_w*(x_neg . W_q)) and the sweep `ps` runs on the positive-range plane
    // alone: half the MFMA work of this pass.
    int fold_negative_plane(Pass& ps) {
        Pass fp = ps;
        fp.twin = false; fp.epi = EPI_STORE; fp.wt_mode = 0; fp.eq_n = 1;
        fp.row = xneg_operand(); fp.row2 = Operand{};
        fp.s1 = ps.s2;
        fp.store_out = Ufold; fp.cache = nullptr;      // (EPI_STORE: planned as a storing pass in the sizing run too, where Ufold is null)
        fp.scores_out = nullptr; fp.best_out = nullptr;
        CHK(run_pass(c, fp));
        ps.twin = false; ps.row2 = Operand{};
        ps.O = Ufold; ps.bias = nullptr;
        // Ufold depends on the CURRENT w_interval: it is rebuilt for every activation pass that runs, so the
        // fragment-order image of k_sweep6's epilogue operands (built from ps.O) must be rebuilt with it
        ps.ecache = nullptr;
        slice.o_src = nullptr;          // ... and so are the gathered rows of the target in the sample slice
        slice2.o_src = nullptr;         // (both tiers: the second one compares the same pointer and would otherwise keep
                                        // the previous pass's target rows when two tier-2 activation passes follow each other)
        return 0;
    }

    // One side of one round: the side's block steps (`memo_on`: the side's pass memo, see memo_of).
    int side_passes(int side, int round, bool memo_on) {
        const bool ws = side == 0;
        const int nblk = ws ? nH : nA;
        for (int blk = 0; blk < nblk; ++blk) {
            if (only_blk >= 0 && blk != only_blk) continue;
            if (segcos) { Pass ps = seg_cos_pass(side, round, blk); CHK(run_pass(c, ps)); continue; }
            const float* cands = ws ? w_cands : a_cands;
            if (general && nblk > 1) { CHK(mix_candidates(side, blk)); cands = ws ? w_mix : a_mix; }
            Pass ps = search_pass(side, round, blk, cands, memo_on);
            if (!ws && twin && wt_mode <= 1) CHK(fold_negative_plane(ps));
            CHK(run_pass_pruned(c, ps));
        }
        return 0;
    }
    // With n_H > 1 the weight search is a coordinate descent over the column blocks: block h is swept with the other
    // blocks at the interval ENTERING the pass (linear.py:468), so its result also depends on w_iv, not only on a_iv
    // (same for n_a > 1 and the activation search).  The memo keys on the counterpart interval alone (just read back / written by
    // the last pass: search_rounds takes the host copies) and is therefore only used where that is the whole input of the pass:
    // the side has ONE block.
    bool memo_of(int side) const { return rounds.memo_on && (side == 0 ? nH : nA) == 1; }
    SearchSide search_side(int side) {
        const DevVecs w(t.w_iv, nV * nH), a(t.a_iv, nA);
        const bool on = memo_of(side);
        return SearchSide(side == 0 ? ST_S1 : ST_S2, on, side == 0 ? a : w, side == 0 ? w : a, [this, side, on](int round) { return side_passes(side, round, on); });
    }
};

int linear_impl(const p4v_linear_desc* d, const LinearTensors& t, const Stage& sg, Ctx& c) {
    LinearCall L(c, d, t, sg);
    CHK(L.build());
    // (the weight side first: it depends on no captured tensor -- inside a group that was handed a "capture done" event it runs,
    // with the candidate planes of the weights further down, while the capture passes are still on the GPU)
    CHK(L.init_side(0));
    if (!sg.full()) {                            // (quant_forward, the granular entry points: no capture to overlap with)
        CHK(q_wait_inputs(c));
        CHK(L.init_side(1));
    }
    if (sg.forward()) { Pass fp = L.forward_pass(); return run_pass(c, fp); }
    if (!sg.searches()) return 0;
    const SearchRounds& R = L.rounds;
    MirrorScope mirrors(c, R.memo_on, t.w_iv, t.a_iv);
    SearchSide sides[2] = {L.search_side(0), L.search_side(1)};
    HostCopy host[2];                            // host copies of w_iv / a_iv, when a pass just moved them
    if (sg.full()) {
        // The 100 candidate planes of the weights (8.5 GB per ViT-B calibration over its 48 Linear layers) need the weights and
        // their candidate table, nothing captured: packed here, before the call waits for its captured tensors.
        if (R.keep_planes && L.nH == 1 && !L.cosm && (sg.mask & ST_S1)) {
            Pass pp = L.search_pass(0, 0, 0, L.w_cands, R.memo_on);
            pp.pack_only = true;
            CHK(run_pass(c, pp));
        }
        CHK(q_wait_inputs(c));
        CHK(L.init_side(1));
    }
    if (L.segcos) CHK(enqueue(c, KERN(NchwRowsParams, k_nchw_to_rows), dim3(cdiv(L.N, 32), cdiv(L.M, 32), 1), dim3(256), 0, NchwRowsParams{t.O, L.M, L.N, L.Ot}));
    return search_rounds(c, R, sg, sides, host);
}

// ------------------------------------------------------------------------------------------------
// Fused forwards: a producer kernel writes the int8 row plane(s) the consumer's forward pass reads
// ------------------------------------------------------------------------------------------------
// Where the planes of the calling thread's last call lie in its workspace (p4v_debug_mlp_planes / p4v_debug_attn_planes: the
// tests read them there)
struct FusedPlanes { size_t off1 = 0, off2 = 0; long rows = 0, cols = 0; int twin = 0; };
thread_local FusedPlanes g_mlp_planes, g_attn_planes;
// ... and the three operand planes k_qkv_heads wrote (p4v_debug_qkv_planes): offsets, then Z and the planes' rows / row lengths
struct QkvPlanes { size_t off_q = 0, off_k = 0, off_v = 0; long Z = 0, rows_q = 0, rows_k = 0, ld_qk = 0, rows_v = 0, ld_v = 0; };
thread_local QkvPlanes g_qkv_planes;
constexpr int MLP_RECORD_KIND = 16, ATTN_RECORD_KIND = 17, QKV_RECORD_KIND = 18;

// One producer -> consumer chain, in the order its caller walks it: plan_consumer, produce, consume.
struct FusedChain {
    struct Packed { char *rows, *cols; float* S1; int Kp, Np; };    // the producer's operand planes [Z][Mp | Np][Kp] and its scale table
    struct PrePlanes { char *rows, *cols, *col2; };                 // planes an earlier launch wrote: the producer's two, the consumer's column plane
    static int producer_kp(int K1) { return (int)rup(K1, 64); }
    static int producer_np(int ncols) { return (int)rup(ncols, SW_BN); }
    // Both operands of a forward pass `fp1` (reduction length K1, `ncols` columns, `nscale` scale entries; rows padded to Mp_) and
    // its scale table as run_pass would make them (pack_operand, k_scale_table), in scratch of the bump region.  With `pre` the
    // planes are taken as they are: only the scale table is made.
    static int pack_pair(Ctx& c, Pass& fp1, int Z_, int Mp_, int K1, int ncols, int nscale, Packed& pk, const PrePlanes* pre = nullptr) {
        pk.Kp = producer_kp(K1); pk.Np = producer_np(ncols);
        SweepPlan pl1{};                                            // what pack_operand reads of a plan: the plane geometry
        pl1.esz = 1; pl1.Mp = Mp_; pl1.Np = pl1.NpB = pk.Np; pl1.Kp = pk.Kp; pl1.cin_fix = 0;
        pk.rows = pre ? pre->rows : c.ws.get<char>((size_t)Z_ * Mp_ * pk.Kp);
        pk.cols = pre ? pre->cols : c.ws.get<char>((size_t)Z_ * pk.Np * pk.Kp);
        pk.S1 = c.ws.get<float>((size_t)nscale);
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", c.ws.off);
        fp1.s1.S = pk.S1; fp1.s1.C = 1; fp1.s1.nblk = fp1.s_cs;
        CHK(launch_scale(c, fp1.s1));
        if (pre) return 0;
        const PassBufs nb{};
        CHK(pack_operand(c, fp1, pl1, nb, fp1.row, pk.rows, false, 0, 1));
        CHK(pack_operand(c, fp1, pl1, nb, fp1.col, pk.cols, true, 0, 1));
        return 0;
    }
    Ctx& c;
    const char *who, *consumer;                                     // for the messages: "mlp" / "attn", "fc2" / "p v"
    Pass fp2{};                                                     // the consumer's forward pass
    SweepPlan pl2{};
    int Z = 1, Mp = 0, Kp = 0;                                      // the consumer's row plane(s): [Z][Mp][Kp] int8
    bool twin = false;
    char *P1 = nullptr, *P2 = nullptr;                              // (null in the sizing run: it carves nothing)

    // The consumer's pass first: its plan says how large the row plane(s) are.
    int plan_consumer(const Pass& fwd, int Z_, bool twin_) {
        fp2 = fwd; Z = Z_; twin = twin_;
        CHK(plan_sweep(c, fp2, pl2));
        if (pl2.cin_fix != 0 || pl2.merged7 || pl2.esz != 1) return fail(P4V_ERR_UNSUPPORTED, "%s: %s's sweep does not read row-major int8 planes", who, consumer);
        Mp = pl2.Mp; Kp = pl2.Kp;
        P1 = c.ws.get<char>((size_t)Z * Mp * Kp);
        P2 = twin ? c.ws.get<char>((size_t)Z * Mp * Kp) : nullptr;
        return 0;
    }
    // The producer: both operands of its forward pass `fp1` (reduction length K1, `ncols` columns, `nscale` scale entries) packed
    // as run_pass would pack them (pack_operand, k_scale_table) into scratch that is given back at the end, then -- unless the
    // run is dry -- `launch(Packed)`, which enqueues the kernel that writes P1 / P2.
    // `pre` (qkv_attn_impl): the producer's operand planes are on the stream already, in this geometry -- nothing is packed.
    template <class Launch> int produce(Pass fp1, int K1, int ncols, int nscale, FusedPlanes& where, Launch&& launch, const PrePlanes* pre = nullptr) {
        const size_t mark = c.ws.off;
        Packed pk{};
        CHK(pack_pair(c, fp1, Z, Mp, K1, ncols, nscale, pk, pre));
        if (!c.dry) {
            CHK(launch(pk));
            where = FusedPlanes{(size_t)(P1 - c.ws.base), P2 ? (size_t)(P2 - c.ws.base) : 0, (long)Z * Mp, Kp, twin ? 1 : 0};
        }
        c.ws.off = mark;
        return 0;
    }
    // The consumer's pass as run_pass runs it, the row operand prepacked (Operand.prepacked): same sweep kernel, same epilogue.
    // `pre` (qkv_attn_impl): the column operand's plane [Z][pl2.NpB][pl2.Kp] is on the stream too.
    int consume(const PrePlanes* pre = nullptr) {
        fp2.row.prepacked = true; fp2.row.plane = P1;
        if (twin) { fp2.row2.prepacked = true; fp2.row2.plane = P2; }
        if (pre) { fp2.col.prepacked = true; fp2.col.plane = pre->col2; }
        return run_pass(c, fp2);
    }
};
// the dry run of the planner: the envelope's verdict, and the bytes the call needs
template <class D, class T> int fused_sizing_run(int (*impl)(const D*, const T&, const T&, Ctx&), const D* d, size_t* need) {
    Ctx c = Ctx::sizing();
    CHK(impl(d, T{}, T{}, c));
    *need = c.sized_bytes();
    return 0;
}
// A fused entry point behind its pointer checks.  The producer's launches precede the planning of the consumer's pass: the whole
// need is checked here, before the first of them.
template <class D, class T> int fused_call(int (*impl)(const D*, const T&, const T&, Ctx&), const D* d, const T& t1, const T& t2, void* d_ws,
                                           size_t ws_bytes, void* stream) {
    size_t need = 0;
    CHK(fused_sizing_run(impl, d, &need));
    if (ws_bytes < need) return fail(P4V_ERR_WORKSPACE, "workspace too small: need >= %zu bytes", need);
    Ctx c = Ctx::on(stream, d_ws, ws_bytes);
    return impl(d, t1, t2, c);
}

// ---- p4v_mlp_quant_forward: fc1 -> GELU -> fc2's activation quantiser -> fc2 with int8 in between ------------------------------
// The producer is k_mlp_fc1 on x and W1: its epilogue writes fc2's row plane(s) -- the fp32 hidden tensor, torch's GELU over it
// and k_pack_dual / k_pack1 of it are gone.
// `t1`, `t2`: the two layers' records as p4v_linear_quant_forward fills them -- t1.fwd_out is the optional fp32 copy of the hidden
// tensor (fc1 stores no other output), t2.X stays null (fc2 reads fc1's planes).
int mlp_impl(const p4v_mlp_desc* d, const LinearTensors& t1, const LinearTensors& t2, Ctx& c) {
    const p4v_linear_desc* d1 = &d->fc1;
    const p4v_linear_desc* d2 = &d->fc2;
    // the envelope, before anything is planned or launched
    if ((long)d1->batch * d1->tokens != (long)d2->batch * d2->tokens || d1->out_features != d2->in_features)
        return fail(P4V_ERR_INVALID, "mlp: fc1's output [%ld][%d] is not fc2's input [%ld][%d]", (long)d1->batch * d1->tokens, d1->out_features,
                    (long)d2->batch * d2->tokens, d2->in_features);
    if (d1->n_H != 1 || d1->n_a != 1 || d2->n_H != 1 || d2->n_a != 1)
        return fail(P4V_ERR_UNSUPPORTED, "mlp: the fused forward takes n_H = n_a = 1 on both layers");
    if (d1->twin_postgelu) return fail(P4V_ERR_UNSUPPORTED, "mlp: fc1 reads no GELU output (twin_postgelu belongs on fc2)");
    if ((d1->reserved | d2->reserved) & RSV_FP32_PLANES) return fail(P4V_ERR_UNSUPPORTED, "mlp: int8 planes only (desc.reserved bit 0 is set)");
    const Stage sg{ST_FWD};
    LinearCall L1(c, d1, t1, sg), L2(c, d2, t2, sg);
    CHK(L1.build());
    CHK(L2.build());
    if (!L1.i8 || !L2.i8) return fail(P4V_ERR_UNSUPPORTED, "mlp: int8 planes only");
    FusedChain ch{c, "mlp", "fc2"};
    CHK(ch.plan_consumer(L2.forward_pass(), 1, L2.twin));      // Kp = roundup64(hidden)
    const int M = L1.M, K1 = L1.K, Hd = L1.N;
    CHK(ch.produce(L1.forward_pass(), K1, Hd, L1.nV, g_mlp_planes, [&](const FusedChain::Packed& pk) -> int {
        MlpFc1Params q{};
        q.A = pk.rows; q.B = pk.cols; q.ldk = pk.Kp; q.ktiles = pk.Kp / SW_BKB;
        q.S1 = pk.S1; q.s_cs = L1.nV; q.sb_div = L1.crb_rows;
        q.bias = t1.bias; q.M = M; q.N = Hd; q.mtiles = ch.Mp / SW_BM; q.ntiles = pk.Np / SW_BN;
        q.q1 = t2.a_iv; q.q2 = nullptr; q.q2_const = L2.a_neg;
        q.lo1 = L2.twin ? 0 : -L2.aq; q.hi1 = L2.aq - 1; q.lo2 = -L2.aq; q.hi2 = 0;
        q.P1 = (int8_t*)ch.P1; q.P2 = (int8_t*)ch.P2; q.Kp = ch.Kp; q.hidden = t1.fwd_out;
        g_alg_macs_cand = (double)M * Hd * K1;
        g_alg_bytes = 4.0 * ((double)M * K1 + (double)Hd * K1) + (double)M * Hd * (L2.twin ? 2 : 1);
        g_exec_frac = 1.0;
        const StatInfo si = stat_info(MLP_RECORD_KIND, (double)ch.Mp * pk.Np * pk.Kp, g_alg_macs_cand, q.mtiles * q.ntiles, 1, g_alg_bytes);
        const dim3 grid(q.mtiles * q.ntiles), block(512);
        const size_t lds = 2 * 2 * SW_TILE_BYTES;
        return L2.twin ? enqueue(c, KERN1_T(MlpFc1Params, k_mlp_fc1, true), grid, block, lds, q, &si)
                       : enqueue(c, KERN1_T(MlpFc1Params, k_mlp_fc1, false), grid, block, lds, q, &si);
    }));
    return ch.consume();
}

// ------------------------------------------------------------------------------------------------
// MatMul
// ------------------------------------------------------------------------------------------------
// Row / column sub-blocks of the (n_G, n_V, n_H) view (reference matmul.py:109-138); (v, h): the block of a granular step
// (all counts 1, the default: no sub-blocks -- the head-wise engine)
struct MatMulBlocks {
    int nVA = 1, nHA = 1, nVB = 1, nHB = 1, v = 0, h = 0;
    bool any() const { return nVA != 1 || nHA != 1 || nVB != 1 || nHB != 1; }
};
MatMulBlocks blocks_of(const p4v_matmul_blocks_desc* d, int v = 0, int h = 0) { return MatMulBlocks{d->n_V_A, d->n_H_A, d->n_V_B, d->n_H_B, v, h}; }
int blocks_check(const p4v_matmul_blocks_desc* d, const char* who, const char* what = "") {
    if (d->n_V_A < 1 || d->n_H_A < 1 || d->n_V_B < 1 || d->n_H_B < 1) return fail(P4V_ERR_INVALID, "%s: %snon-positive block count", who, what);
    return 0;
}
// The device pointers of one matmul_impl call, filled by name at the entry points; what the call's mode (Stage) does not read
// stays null, and a sizing run leaves all of them null.
struct MatMulTensors {
    const float *A = nullptr, *B = nullptr;                     // the operands, read through the descriptor's strides
    const float *O = nullptr, *G = nullptr;                     // raw_out / raw_grad [Z][M][N] (searches; G: the hessian metric)
    const float* mult = nullptr;                                // [eq_n + 1] candidate multipliers (ST_INIT with a search)
    float *A_iv = nullptr, *B_iv = nullptr;                     // intervals [heads] (sub-blocks: [heads][n_V][n_H]; sos: the scalar A_interval)
    float* split = nullptr;                                     // sos: the split -- out of the split search, in for the B search and ST_FWD
    float* scores = nullptr; int32_t* best = nullptr;           // optional score tables / selections
    float* fwd_out = nullptr;                                   // ST_FWD: the destination [Z][M][N]
};
// The argument checks of every matmul_impl call, with or without sub-blocks (the block counts are checked after them:
// MatMulBlocksCall::build)
int matmul_check(const p4v_matmul_desc* d, const MatMulTensors& t, const Stage& sg, const Ctx& c) {
    if (d->batch * d->heads <= 0 || d->M <= 0 || d->K <= 0 || d->N <= 0 || d->eq_n <= 0) return fail(P4V_ERR_INVALID, "matmul: non-positive dimension");
    if (d->A_bit > 8 || d->B_bit > 8 || d->A_bit < 2 || d->B_bit < 2) return fail(P4V_ERR_UNSUPPORTED, "matmul: bit widths 2..8 supported");
    int epi, wt_mode;
    metric_epi(d->metric, &epi, &wt_mode);
    if (wt_mode == 1 && !t.G && sg.searches() && !c.dry) return fail(P4V_ERR_INVALID, "matmul: hessian metric needs raw_grad");
    // the split: written by the split search, read by the B search and the forward; the initialisation alone does without
    if (d->sos && !t.split && (sg.searches() || sg.forward()) && !c.dry) return fail(P4V_ERR_INVALID, "matmul: sos needs d_split");
    return 0;
}

// One head-wise matmul_impl call: geometry, workspace and the builders of its passes.  Sides: 0 = the A search (with sos: the
// split search), 1 = the B search.
struct MatMulCall {
    static constexpr int NSPLIT = 20;                 // matmul.py:636
    Ctx& c;
    const p4v_matmul_desc* d;
    const MatMulTensors t;
    const Stage& sg;
    int H = 0, Z = 0, M = 0, K = 0, N = 0;            // heads, batch x heads, the GEMM of one head
    int Aq = 0, Bq = 0;                               // 2^(bit - 1)
    int epi = 0, wt_mode = 0, ncand = 0;
    bool cosm = false;
    unsigned *enc_A = nullptr, *enc_B = nullptr;
    float *A_cands_ws = nullptr, *B_cands_ws = nullptr;
    const float *A_cands = nullptr, *B_cands = nullptr;         // built by this call, or the caller's (granular search)
    float* split_cands = nullptr;                     // 2^-i, i < NSPLIT
    float* A_headwise = nullptr;                      // sos: the inherited head-wise A interval is computed then overwritten (matmul.py:419-440)
    SearchRounds rounds;
    PlaneCache plane_A, plane_B;
    SliceCache slice;

    MatMulCall(Ctx& c_, const p4v_matmul_desc* d_, const MatMulTensors& t_, const Stage& sg_) : c(c_), d(d_), t(grad_by_metric(t_, d_->metric)), sg(sg_) {}

    // geometry of a call that passed matmul_check
    void build() {
        H = d->heads; Z = d->batch * d->heads; M = d->M; K = d->K; N = d->N;
        Aq = 1 << (d->A_bit - 1); Bq = 1 << (d->B_bit - 1);
        metric_epi(d->metric, &epi, &wt_mode);
        cosm = epi == EPI_COS;
        ncand = d->eq_n + 1;
        rounds = SearchRounds(sg, d->search_round, !(d->reserved & RSV_NO_MEMO), d->eq_n, H, c, t.scores, t.best);
    }
    int workspace() {
        enc_A = c.ws.get<unsigned>(H);
        enc_B = c.ws.get<unsigned>(H);
        A_cands_ws = c.ws.get<float>((size_t)ncand * H);
        B_cands_ws = c.ws.get<float>((size_t)ncand * H);
        A_cands = sg.inits() ? A_cands_ws : sg.cands1;
        B_cands = sg.inits() ? B_cands_ws : sg.cands2;
        split_cands = c.ws.get<float>(NSPLIT);
        A_headwise = c.ws.get<float>(H);
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small");
        return 0;
    }
    // interval initialisation of both operands and their candidate tables
    int init() {
        if (!sg.inits()) return 0;
        const long sa[4] = {d->a_stride[0], d->a_stride[1], d->a_stride[2], d->a_stride[3]};
        const long sb[4] = {d->b_stride[0], d->b_stride[1], d->b_stride[2], d->b_stride[3]};
        float* a_dst = d->sos ? A_headwise : t.A_iv;
        CHK(launch_absmax(c, t.A, sa, d->batch, H, M, K, 1, 1, M, K, 0, enc_A));
        CHK(launch_interval(c, enc_A, H, (float)(Aq - 0.5), d->init_layerwise, a_dst));
        CHK(launch_absmax(c, t.B, sb, d->batch, H, K, N, 1, 1, K, N, 0, enc_B));
        CHK(launch_interval(c, enc_B, H, (float)(Bq - 0.5), d->init_layerwise, t.B_iv));
        if (sg.searches()) {
            if (!d->sos) CHK(launch_cands(c, t.mult, t.A_iv, ncand, H, A_cands_ws));
            CHK(launch_cands(c, t.mult, t.B_iv, ncand, H, B_cands_ws));
        }
        return 0;
    }
    // the split candidates 2**(-i) of the split-of-softmax search
    int upload_splits() {
        if (!(sg.mask & ST_S1) || !d->sos || c.dry) return 0;
        float sc[NSPLIT];
        for (int i = 0; i < NSPLIT; ++i) sc[i] = (float)std::ldexp(1.0, -i);  // 2**(-i), exact in fp32
        CHK(q_h2d(c, split_cands, sc, sizeof sc));
        if (!c.grp) CHK(q_sync(c));          // sc lives on this stack frame (a group's queue holds a copy)
        return 0;
    }

    // logical [Z][rows][K] views: A rows = m, B rows = n (B given as [K][N])
    Operand operand(const float* src, const int64_t* st, int r_ax, int k_ax, int R, int q, bool expanded, const float* scales, int sc_cs, int mode) const {
        Operand op{};
        op.present = true; op.expanded = expanded;
        op.pk = PackParams{};
        op.pk.src = src; op.pk.s_z = st[1]; op.pk.s_r = st[r_ax]; op.pk.s_k = st[k_ax];
        op.pk.s_z2 = st[0]; op.pk.zdiv = H;
        op.pk.Z = Z; op.pk.R = R; op.pk.K = K; op.pk.nblk_r = 1; op.pk.nblk_k = 1;
        op.pk.mode = mode; op.pk.scales = scales; op.pk.sc_cs = sc_cs;
        op.pk.blk_mode = (mode == PACK_SYM) ? 2 : 0; op.pk.blk_div = H;
        op.pk.lo = -q; op.pk.hi = q - 1;
        return op;
    }
    Operand A_operand(bool expanded, const float* scales, int sc_cs, int mode) const {
        Operand op = operand(t.A, d->a_stride, 2, 3, M, Aq, expanded, scales, sc_cs, mode);
        op.pk.qm1 = (float)(Aq - 1);
        return op;
    }
    Operand B_operand(bool expanded, const float* scales, int sc_cs, int mode) const {
        return operand(t.B, d->b_stride, 3, 2, N, Bq, expanded, scales, sc_cs, mode);
    }
    // what every search pass shares: the GEMM and its target; cosine runs swapped (rows = n)
    void common(Pass& ps) const {
        ps.Z = Z; ps.K = K;
        ps.O = t.O; ps.G = t.G; ps.wt_mode = wt_mode; ps.epi = epi;
        ps.o_inner = INT_MAX;
        if (!cosm) { ps.Mrows = M; ps.Ncols = N; ps.o_zs = (long)M * N; ps.o_ms = N; ps.o_ns = 1; }
        else { ps.Mrows = N; ps.Ncols = M; ps.o_zs = (long)M * N; ps.o_ms = 1; ps.o_ns = N; ps.G = nullptr;
               ps.cos_ZB = Z; ps.cos_ZV = 1; }
    }
    // A on the rows and B on the columns, or swapped for cosine
    void place(Pass& ps, const Operand& a, const Operand& b) const {
        if (!cosm) { ps.row = a; ps.col = b; } else { ps.row = b; ps.col = a; }
    }
    // ... and one score, one candidate column, one interval per head
    void per_head(Pass& ps, const float* cands, float* interval) const {
        ps.j_mode = 2; ps.j_div = H; ps.nj = H; ps.cos_j_mode = 2; ps.cos_j_div = H;
        ps.norm = cosm ? 1.0 / (double)M : 1.0 / ((double)M * N);
        ps.cands = cands; ps.cand_cs = H; ps.cand_js = 1; ps.interval = interval; ps.out_js = 1;
        ps.scores_out_ld = H;
    }

    Pass forward_pass() const {
        Pass fp{};
        fp.Z = Z; fp.K = K; fp.Mrows = M; fp.Ncols = N;
        fp.i8 = true; fp.twin = d->sos; fp.epi = EPI_FWD; fp.wt_mode = 0; fp.eq_n = 1;
        fp.row = d->sos ? A_operand(false, t.split, 0, PACK_SOS_HI) : A_operand(false, t.A_iv, 0, PACK_SYM);
        if (d->sos) fp.row2 = A_operand(false, t.split, 0, PACK_SOS_LO);
        fp.col = B_operand(false, t.B_iv, 0, PACK_SYM);
        fp.use_s1 = true; fp.s_cs = H; fp.sb_mode = 2; fp.sb_div = H;
        if (!d->sos) fp.s1 = ScaleParams{t.A_iv, 0, 1, 0.f, t.B_iv, 0, 1, 0.f, 0, 0, nullptr};
        else {
            fp.s1 = ScaleParams{nullptr, 0, 0, 1.0f / (float)(Aq - 1), t.B_iv, 0, 1, 0.f, 0, 0, nullptr};
            fp.s2 = ScaleParams{t.A_iv, 0, 0, 0.f, t.B_iv, 0, 1, 0.f, 0, 0, nullptr};
        }
        fp.O = t.fwd_out; fp.G = nullptr; fp.o_zs = (long)M * N; fp.o_ms = N; fp.o_ns = 1; fp.o_inner = INT_MAX;
        fp.nj = 1; fp.store_out = t.fwd_out;
        return fp;
    }
    // A search, B fixed at its current head-wise interval (matmul.py:483-522)
    Pass A_pass(int round) {
        Pass ps{};
        common(ps);
        ps.i8 = true; ps.twin = false; ps.eq_n = d->eq_n;
        place(ps, A_operand(true, A_cands, H, PACK_SYM), B_operand(false, t.B_iv, 0, PACK_SYM));
        ps.use_s1 = true; ps.s_cs = H; ps.sb_mode = 2; ps.sb_div = H;
        ps.s1 = ScaleParams{A_cands, H, 1, 0.f, t.B_iv, 0, 1, 0.f, 0, 0, nullptr};
        per_head(ps, A_cands, t.A_iv);
        ps.cache = rounds.keep_planes ? &plane_A : nullptr;
        ps.scores_out = rounds.scores_of(round, 0); ps.best_out = rounds.best_of(round, 0);
        ps.prunable = !cosm && !(d->reserved & RSV_NO_PRUNE); ps.scache = &slice; ps.host_sync_ok = rounds.memo_on;
        return ps;
    }
    // split search against the UNQUANTISED B (matmul.py:600-631): A quantised in registers, one kernel (k_sos_split)
    SosSplitJob split_job(int round) {
        SosSplitJob j{};
        j.kp.A = t.A; j.kp.a_z2 = d->a_stride[0]; j.kp.a_z = d->a_stride[1]; j.kp.a_r = d->a_stride[2]; j.kp.a_k = d->a_stride[3];
        j.kp.zdiv = H;
        j.kp.B = t.B; j.kp.b_z2 = d->b_stride[0]; j.kp.b_z = d->b_stride[1]; j.kp.b_k = d->b_stride[2]; j.kp.b_n = d->b_stride[3];
        j.kp.O = t.O; j.kp.G = t.G ? t.G : t.O;
        j.kp.Z = Z; j.kp.M = M; j.kp.K = K; j.kp.N = N; j.kp.wt_mode = wt_mode; j.kp.C = NSPLIT;
        j.kp.splits = split_cands;
        j.kp.qm1 = (float)(Aq - 1); j.kp.c_inv = 1.0f / (float)(Aq - 1);
        j.kp.lo_top = std::min(std::nearbyintf(1.0f / j.kp.c_inv), (float)(Aq - 1));
        j.kp.halves = cdiv(M, 128);
        j.epi = epi; j.norm = 1.0 / ((double)H * M * N);
        j.cands = split_cands; j.split = t.split; j.A_iv = t.A_iv; j.aux_div = (float)(Aq - 1);   // A_interval = split/(qmax-1) (matmul.py:629)
        j.scores_out = (d->eq_n >= NSPLIT) ? rounds.scores_of(round, 0) : nullptr; j.scores_out_ld = H; j.best_out = rounds.best_of(round, 0);
        j.scache = &slice; j.host_sync_ok = rounds.memo_on; j.prunable = !(d->reserved & RSV_NO_PRUNE);
        return j;
    }
    // ... the same search on fp32 operands (shapes k_sos_split has no instance for, cosine)
    Pass split_pass_f32(int round) {
        Pass ps{};
        common(ps);
        ps.i8 = false; ps.twin = false; ps.eq_n = NSPLIT;
        place(ps, A_operand(true, split_cands, 1, PACK_SOS_SIM), B_operand(false, nullptr, 0, PACK_RAW));
        ps.use_s1 = false; ps.s_cs = 1; ps.sb_mode = 0;
        ps.j_mode = 0; ps.nj = 1; ps.cos_j_mode = 0;
        ps.norm = cosm ? 1.0 / ((double)H * M) : 1.0 / ((double)H * M * N);
        ps.cands = split_cands; ps.cand_cs = 1; ps.cand_js = 0; ps.interval = t.split; ps.out_js = 0;
        ps.aux_out = t.A_iv; ps.aux_div = (float)(Aq - 1);   // A_interval = split/(qmax-1) (matmul.py:629)
        ps.scores_out = (d->eq_n >= NSPLIT) ? rounds.scores_of(round, 0) : nullptr; ps.scores_out_ld = H; ps.best_out = rounds.best_of(round, 0);
        return ps;
    }
    // B search, A fixed (matmul.py:524-563); with sos, A is the two-range twin (matmul.py:595-598)
    Pass B_pass(int round) {
        Pass ps{};
        common(ps);
        ps.eq_n = d->eq_n;
        const bool twin_rows = d->sos && !cosm;
        ps.i8 = !(d->sos && cosm);   // cosine + sos: fp32 operands (the twin sits on the column side when swapped)
        ps.twin = twin_rows;
        place(ps, d->sos ? A_operand(false, t.split, 0, ps.i8 ? PACK_SOS_HI : PACK_SOS_SIM) : A_operand(false, t.A_iv, 0, PACK_SYM),
              B_operand(true, B_cands, H, PACK_SYM));
        if (twin_rows) ps.row2 = A_operand(false, t.split, 0, PACK_SOS_LO);
        ps.use_s1 = ps.i8; ps.s_cs = H; ps.sb_mode = 2; ps.sb_div = H;
        if (!d->sos) ps.s1 = ScaleParams{t.A_iv, 0, 1, 0.f, B_cands, H, 1, 0.f, 0, 0, nullptr};
        else {
            // high range: k_hi/(q-1) ; low range: k_lo * (split/(q-1)) = k_lo * A_interval
            ps.s1 = ScaleParams{nullptr, 0, 0, 1.0f / (float)(Aq - 1), B_cands, H, 1, 0.f, 0, 0, nullptr};
            ps.s2 = ScaleParams{t.A_iv, 0, 0, 0.f, B_cands, H, 1, 0.f, 0, 0, nullptr};
        }
        per_head(ps, B_cands, t.B_iv);
        ps.cache = rounds.keep_planes ? &plane_B : nullptr;
        ps.scores_out = rounds.scores_of(round, 1); ps.best_out = rounds.best_of(round, 1);
        ps.prunable = !cosm && ps.i8 && !(d->reserved & RSV_NO_PRUNE); ps.scache = &slice; ps.host_sync_ok = rounds.memo_on;
        return ps;
    }
    // The passes of one side of one round.  The A side has three variants: the head-wise A search; with sos the split search on
    // k_sos_split, or on fp32 operands where that kernel has no instance.
    int side_passes(int side, int round) {
        if (side == 1) { Pass ps = B_pass(round); return run_pass_pruned(c, ps); }
        if (!d->sos) { Pass ps = A_pass(round); return run_pass_pruned(c, ps); }
        if (sos_split_ok(M, K, N, cosm)) {
            SosSplitJob j = split_job(round);
            if (g_sos_debug) return c.grp || c.dry ? fail(P4V_ERR_INVALID, "p4v_debug_sos_sweep: not inside a group") : run_sos_debug_sweep(c, j, *g_sos_debug);
            return run_sos_split_pruned(c, j);
        }
        Pass ps = split_pass_f32(round);
        return run_pass(c, ps);
    }
    // the A search is a function of B's interval; with sos it is the split search against the RAW B: a function of nothing ->
    // always a hit after round 1, its value the split and the A interval derived from it
    SearchSide search_side(int side) {
        const int nAiv = d->sos ? 1 : H;
        const DevVecs A_key = d->sos ? DevVecs() : DevVecs(t.B_iv, H), A_val = d->sos ? DevVecs(t.split, 1, t.A_iv, 1) : DevVecs(t.A_iv, nAiv);
        auto run = [this, side](int round) { return side_passes(side, round); };
        return side == 0 ? SearchSide(ST_S1, rounds.memo_on, A_key, A_val, run) : SearchSide(ST_S2, rounds.memo_on, DevVecs(t.A_iv, nAiv), DevVecs(t.B_iv, H), run);
    }
    // the head-wise call, after matmul_impl's checks and its wait for the inputs
    int run() {
        build();
        CHK(workspace());
        CHK(init());
        if (sg.forward()) { Pass fp = forward_pass(); return run_pass(c, fp); }
        if (!sg.searches()) return 0;
        CHK(upload_splits());
        MirrorScope mirrors(c, rounds.memo_on, t.A_iv, t.B_iv, d->sos ? t.split : nullptr);
        SearchSide sides[2] = {search_side(0), search_side(1)};
        return search_rounds(c, rounds, sg, sides, nullptr);
    }
};

// ---- p4v_attn_quant_forward: matmul1 -> * scale -> softmax -> matmul2's A quantiser -> matmul2, int8 in between (the FusedChain above)
// The producer is k_attn_qk on q and k^T: it writes matmul2's row plane(s) ([Z][Mp][Kp]: the tiled sweeps step Mp * Kp per z, the
// plane's own layout) -- the fp32 score tensor, torch's `* scale` and softmax over it and k_pack_dual of it are gone.
// `t1`, `t2`: the two MatMuls' records as p4v_matmul_quant_forward fills them -- t1.fwd_out is the optional fp32 copy of the
// probabilities [Z][M][N] (matmul1 stores no other output), t2.A stays null (matmul2 reads k_attn_qk's planes).
// `win` (p4v_wattn_quant_forward; null: the plain call): the window record -- q arrives scaled, the kernel's window instance adds
// the relative-position bias and the shift mask in place of `* scale`; everything else of the chain is the same.
struct AttnWindow { const float* bias; const float* mask; int n_windows; };
// `qkv` (p4v_qkv_attn_quant_forward; null: q, k^T and v arrive as fp32 tensors): the qkv layer in front of the chain.  k_qkv_heads
// -- its int8 GEMM on Q(x) and Q(Wqkv), packed as its forward pass would pack them -- writes matmul1's two operand planes and
// matmul2's column plane: the fp32 qkv tensor, the permute copy of it and the three k_pack1 of q, k^T and v are gone.  The three
// planes are carved behind the consumer's row plane(s), outside every region that is handed back, and zeroed first: the kernel
// writes the bytes of valid elements only.
struct QkvProducer {
    const LinearCall& L;
    const LinearTensors& t;
    int run(Ctx& c, const FusedChain& ch, int H, int Ntok, int D, const MatMulTensors& t1, const MatMulCall& m1, const MatMulTensors& t2,
            const MatMulCall& m2, FusedChain::PrePlanes& pre) const {
        const int Z = ch.Z, K1p = FusedChain::producer_kp(D), Np1 = FusedChain::producer_np(Ntok);
        const size_t nq = (size_t)Z * ch.Mp * K1p, nk = (size_t)Z * Np1 * K1p, nv = (size_t)Z * ch.pl2.NpB * ch.pl2.Kp;
        pre.rows = c.ws.get<char>(nq);
        pre.cols = c.ws.get<char>(nk);
        pre.col2 = c.ws.get<char>(nv);
        const size_t mark = c.ws.off;
        Pass fp = L.forward_pass();
        FusedChain::Packed pk{};
        const int Mp = (int)rup(L.M, SW_BM);
        CHK(FusedChain::pack_pair(c, fp, 1, Mp, L.K, L.N, L.nV, pk));
        if (!c.dry) {
            CHK(q_fill(c, pre.rows, 0, nq));
            CHK(q_fill(c, pre.cols, 0, nk));
            CHK(q_fill(c, pre.col2, 0, nv));
            QkvHeadsParams q{};
            q.A = pk.rows; q.B = pk.cols; q.ldk = pk.Kp; q.ktiles = pk.Kp / SW_BKB;
            q.S1 = pk.S1; q.s_cs = L.nV; q.sb_div = L.crb_rows;
            q.bias = t.bias; q.M = L.M; q.N = L.N; q.mtiles = Mp / SW_BM; q.ntiles = pk.Np / SW_BN;
            q.Ntok = Ntok; q.H = H; q.D = D; q.C = H * D;
            q.iv_q = t1.A_iv; q.iv_k = t1.B_iv; q.iv_v = t2.B_iv;
            q.lo_q = -m1.Aq; q.hi_q = m1.Aq - 1; q.lo_k = -m1.Bq; q.hi_k = m1.Bq - 1; q.lo_v = -m2.Bq; q.hi_v = m2.Bq - 1;
            q.Pq = (int8_t*)pre.rows; q.Pk = (int8_t*)pre.cols; q.Pv = (int8_t*)pre.col2;
            q.rows_q = ch.Mp; q.rows_k = Np1; q.ld_qk = K1p; q.rows_v = ch.pl2.NpB; q.ld_v = ch.pl2.Kp;
            q.qkv_out = t.fwd_out;
            g_alg_macs_cand = (double)L.M * L.N * L.K;
            // x and Wqkv in fp32, the three planes: the fill and the kernel's bytes
            g_alg_bytes = 4.0 * ((double)L.M * L.K + (double)L.N * L.K) + (double)(nq + nk + nv) + (double)L.M * L.N;
            g_exec_frac = 1.0;
            const StatInfo si = stat_info(QKV_RECORD_KIND, (double)Mp * pk.Np * pk.Kp, g_alg_macs_cand, q.mtiles * q.ntiles, 1, g_alg_bytes);
            CHK(enqueue(c, Kern1<QkvHeadsParams, k_qkv_heads>::desc(), dim3(q.mtiles * q.ntiles), dim3(512), 2 * 2 * SW_TILE_BYTES, q, &si));
            g_qkv_planes = QkvPlanes{(size_t)(pre.rows - c.ws.base), (size_t)(pre.cols - c.ws.base), (size_t)(pre.col2 - c.ws.base), Z, ch.Mp, Np1, K1p,
                                     ch.pl2.NpB, ch.pl2.Kp};
        }
        c.ws.off = mark;
        return 0;
    }
};
int attn_chain(const p4v_attn_desc* d, const MatMulTensors& t1, const MatMulTensors& t2, Ctx& c, const AttnWindow* win, const QkvProducer* qkv = nullptr) {
    const p4v_matmul_desc* d1 = &d->qk;
    const p4v_matmul_desc* d2 = &d->pv;
    // the envelope, before anything is planned or launched
    if (win) {
        if (win->n_windows < 1) return fail(P4V_ERR_INVALID, "wattn: n_windows = %d is not positive", win->n_windows);
        if (d1->batch % win->n_windows) return fail(P4V_ERR_INVALID, "wattn: qk.batch = %d is no multiple of n_windows = %d", d1->batch, win->n_windows);
        // (the kernel addresses both tensors with 32-bit element offsets)
        if ((double)std::max(d1->heads, win->n_windows) * d1->M * d1->N >= (double)(1 << 30))
            return fail(P4V_ERR_UNSUPPORTED, "wattn: a bias [%d][%d][%d] or mask [%d][%d][%d] of 2^30 elements or more", d1->heads, d1->M, d1->N,
                        win->n_windows, d1->M, d1->N);
    }
    if (d1->batch != d2->batch || d1->heads != d2->heads || d1->M != d2->M || d1->N != d2->K)
        return fail(P4V_ERR_INVALID, "attn: q k^T [%d][%d][%d][%d] is not the row operand of p v [%d][%d][%d][%d]", d1->batch, d1->heads, d1->M, d1->N,
                    d2->batch, d2->heads, d2->M, d2->K);
    if (d1->sos) return fail(P4V_ERR_UNSUPPORTED, "attn: q k^T is no split-of-softmax operand (sos belongs on p v)");
    if ((d1->reserved | d2->reserved) & RSV_FP32_PLANES) return fail(P4V_ERR_UNSUPPORTED, "attn: int8 planes only (desc.reserved bit 0 is set)");
    if (!(d->scale == d->scale)) return fail(P4V_ERR_INVALID, "attn: scale is NaN");
    const Stage sg{ST_FWD};
    MatMulCall m1(c, d1, t1, sg), m2(c, d2, t2, sg);
    CHK(matmul_check(d1, t1, sg, c));
    m1.build();
    CHK(matmul_check(d2, t2, sg, c));
    m2.build();
    cvt_bias(c);     // (first call of the process: probe the conversion quant16_sat8 relies on)
    CHK(q_wait_inputs(c));
    const int Z = m1.Z, H = m1.H, M = m1.M, N = m1.N, K1 = m1.K;
    const bool twin = d2->sos != 0;
    FusedChain ch{c, "attn", "p v"};
    CHK(ch.plan_consumer(m2.forward_pass(), Z, twin));         // Kp = roundup64(N)
    if (ch.Mp % SW_BM || (long)Z * (ch.Mp / SW_BM) >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "attn: %d x %d row tiles", Z, ch.Mp / SW_BM);
    FusedChain::PrePlanes planes{};
    const FusedChain::PrePlanes* pre = qkv ? &planes : nullptr;
    if (qkv) CHK(qkv->run(c, ch, H, N, K1, t1, m1, t2, m2, planes));
    CHK(ch.produce(m1.forward_pass(), K1, N, H, g_attn_planes, [&](const FusedChain::Packed& pk) -> int {
        AttnQkParams q{};
        q.Q = pk.rows; q.Kt = pk.cols; q.q_zs = (long)ch.Mp * pk.Kp; q.k_zs = (long)pk.Np * pk.Kp; q.ldk = pk.Kp; q.ktiles = pk.Kp / SW_BKB;
        q.S1 = pk.S1; q.H = H; q.scale = d->scale;
        q.M = M; q.N = N; q.Mp = ch.Mp; q.Kp = ch.Kp;
        q.qs = twin ? t2.split : t2.A_iv; q.qs_headwise = twin ? 0 : 1;
        q.lo = -m2.Aq; q.hi = m2.Aq - 1; q.qm1 = (float)(m2.Aq - 1);
        q.P1 = (int8_t*)ch.P1; q.P2 = (int8_t*)ch.P2; q.probs = t1.fwd_out;
        q.mtiles = ch.Mp / SW_BM; q.nwg = Z * q.mtiles;
        g_alg_macs_cand = (double)Z * M * N * K1;
        g_alg_bytes = 4.0 * ((double)Z * M * K1 + (double)Z * N * K1) + (double)Z * M * N * (twin ? 2 : 1);
        if (win) g_alg_bytes += 4.0 * (double)M * N * (H + (win->mask ? win->n_windows : 0));
        g_exec_frac = 1.0;
        // (three walks over the keys: the maximum, the sum, the write pass)
        const StatInfo si = stat_info(ATTN_RECORD_KIND, 3.0 * (double)Z * ch.Mp * (double)rup(N, 32) * pk.Kp, g_alg_macs_cand, q.nwg, 1, g_alg_bytes);
        const dim3 grid(q.nwg), block(256);
        const size_t lds = (size_t)4 * (twin ? 2 : 1) * 32 * ATTN_OROW;
        if (win) {
            AttnWinParams w{};
            static_cast<AttnQkParams&>(w) = q;
            w.scale = 1.0f;                                        // (not read by the window instances)
            w.bias = win->bias; w.mask = win->mask; w.n_windows = win->n_windows;
            return twin ? enqueue(c, KERN1_T(AttnWinParams, k_attn_qk, true, true), grid, block, lds, w, &si)
                        : enqueue(c, KERN1_T(AttnWinParams, k_attn_qk, false, true), grid, block, lds, w, &si);
        }
        return twin ? enqueue(c, KERN1_T(AttnQkParams, k_attn_qk, true), grid, block, lds, q, &si)
                    : enqueue(c, KERN1_T(AttnQkParams, k_attn_qk, false), grid, block, lds, q, &si);
    }, pre));
    return ch.consume(pre);
}
int attn_impl(const p4v_attn_desc* d, const MatMulTensors& t1, const MatMulTensors& t2, Ctx& c) { return attn_chain(d, t1, t2, c, nullptr); }
// the window call as fused_sizing_run / fused_call take it: the p4v_attn_desc of its two MatMuls and the window record
struct WattnCall { p4v_attn_desc a; AttnWindow w; };
int wattn_impl(const WattnCall* d, const MatMulTensors& t1, const MatMulTensors& t2, Ctx& c) { return attn_chain(&d->a, t1, t2, c, &d->w); }

// ---- p4v_qkv_attn_quant_forward: the qkv layer in front of the attention chain (QkvProducer above) -----------------------------
// The records of the three modules as their own quant_forward entry points fill them: lin.fwd_out is the optional fp32 copy of
// the qkv tensor, m1.fwd_out the optional probabilities; m1.A, m1.B and m2.B stay null (no fp32 q, k^T or v exists).
struct QkvAttnTensors { LinearTensors lin; MatMulTensors m1, m2; };
int qkv_attn_impl(const p4v_qkv_attn_desc* d, const QkvAttnTensors& t, const QkvAttnTensors&, Ctx& c) {
    const p4v_linear_desc* dl = &d->qkv;
    const p4v_matmul_desc* d1 = &d->qk;
    const p4v_matmul_desc* d2 = &d->pv;
    // the envelope of the qkv layer and of its seam with the chain, before anything is planned or launched (attn_chain checks the
    // two MatMuls against each other)
    if (dl->n_H != 1 || dl->n_a != 1) return fail(P4V_ERR_UNSUPPORTED, "qkv_attn: the fused forward takes n_H = n_a = 1 on qkv");
    if (dl->twin_postgelu) return fail(P4V_ERR_UNSUPPORTED, "qkv_attn: qkv reads no GELU output (twin_postgelu)");
    if (dl->reserved & RSV_FP32_PLANES) return fail(P4V_ERR_UNSUPPORTED, "qkv_attn: int8 planes only (qkv.reserved bit 0 is set)");
    if (d1->heads <= 0 || d1->K <= 0 || d1->M <= 0) return fail(P4V_ERR_INVALID, "qkv_attn: non-positive dimension");
    if (d2->N != d1->K || (long)dl->out_features != 3L * d1->heads * d1->K)
        return fail(P4V_ERR_INVALID, "qkv_attn: qkv.out_features = %d, p v's N = %d: not 3 x %d heads x head_dim %d", dl->out_features, d2->N, d1->heads, d1->K);
    if (d1->M != d1->N || d2->K != d1->M || (long)dl->batch * dl->tokens != (long)d1->batch * d1->M)
        return fail(P4V_ERR_INVALID, "qkv_attn: qkv's rows %ld are not %d images of %d = %d = %d tokens", (long)dl->batch * dl->tokens, d1->batch, d1->M,
                    d1->N, d2->K);
    const Stage sg{ST_FWD};
    LinearCall L(c, dl, t.lin, sg);
    CHK(L.build());
    if (!L.i8) return fail(P4V_ERR_UNSUPPORTED, "qkv_attn: int8 planes only");
    if (rup(L.M, SW_BM) / SW_BM * (rup(L.N, SW_BN) / SW_BN) >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "qkv_attn: %d x %d output tiles", L.M, L.N);
    const p4v_attn_desc a{*d1, *d2, d->scale, 0};
    const QkvProducer qkv{L, t.lin};
    return attn_chain(&a, t.m1, t.m2, c, nullptr, &qkv);
}

// ---- MatMul with row / column sub-blocks (n_V, n_H > 1; reference matmul.py:109-138, 419-440, 483-563) -------------------------
// Intervals are [heads][n_V][n_H] (the reference's (1, n_G = heads, 1, n_V, 1, n_H, 1)).  The search is the reference's greedy
// coordinate descent: block (v, h) in product(range(n_V), range(n_H)) order, its candidates mult * INITIAL interval replacing
// that block's scale only, every other block on the interval entering the step, the score the full-output score per head; each
// step is one sweep of the whole operand (no pruning, no pass memo: first version).  Score tables [round][step][eq_n][heads],
// steps = A blocks then B blocks (split-of-softmax: the 20-row split table, then B blocks).
struct MatMulBlocksCall {
    // one step of a round: side 1 / 2 = block (v, h) of A / B; side 0 = the split search of the split-of-softmax class, which
    // knows no blocks; the step's slot of the [round][step] tables
    struct Step { int side, v, h; float* scores; int32_t* best; };
    Ctx& c;
    const p4v_matmul_desc* d;
    const MatMulBlocks mb;
    const MatMulTensors t;
    const Stage& sg;
    const Stage split_stage{ST_S1};                   // the mode of the split step's head-wise call
    int H = 0, Z = 0, M = 0, K = 0, N = 0;            // heads, batch x heads, the GEMM of one head
    int nVA = 1, nHA = 1, nVB = 1, nHB = 1;           // row / column blocks of A and of B
    int nA = 0, nB = 0;                               // intervals per operand: heads x n_V x n_H (sos: the scalar A interval)
    int epi = 0, wt_mode = 0, ncand = 0;
    SegPlan g{};                                      // the K-segmented view of both operands; step_pass sets its override fields
    unsigned *enc_A = nullptr, *enc_B = nullptr;      // abs-max per block, order-preserving encoding
    float *A_cands_ws = nullptr, *B_cands_ws = nullptr;       // candidate tables [eq_n + 1][heads][n_V][n_H], built by this call
    SearchRounds rounds;                              // tables [round][step]

    MatMulBlocksCall(Ctx& c_, const p4v_matmul_desc* d_, const MatMulBlocks& mb_, const MatMulTensors& t_, const Stage& sg_)
        : c(c_), d(d_), mb(mb_), t(grad_by_metric(t_, d_->metric)), sg(sg_) {}

    // the checks of the block counts (after matmul_check), the segment plan
    int build() {
        H = d->heads; Z = d->batch * d->heads; M = d->M; K = d->K; N = d->N;
        nVA = mb.nVA; nHA = mb.nHA; nVB = mb.nVB; nHB = mb.nHB;
        if (nVA < 1 || nHA < 1 || nVB < 1 || nHB < 1) return fail(P4V_ERR_INVALID, "matmul: non-positive block count");
        if (nVA > 8 || nHA > 8 || nVB > 8 || nHB > 8) return fail(P4V_ERR_UNSUPPORTED, "matmul: sub-blocks up to n_V, n_H = 8 are implemented on the GPU");
        if (d->sos && (nVA != 1 || nHA != 1)) return fail(P4V_ERR_INVALID, "matmul: the split-of-softmax operand has no sub-blocks (matmul.py:586-588)");
        if (d->A_bit < 2 || d->B_bit < 2) return fail(P4V_ERR_UNSUPPORTED, "matmul: bit widths 2..8 supported");
        metric_epi(d->metric, &epi, &wt_mode);
        if (epi == EPI_COS && sg.searches())
            return fail(P4V_ERR_UNSUPPORTED, "matmul: the cosine metric with row/column sub-blocks (n_V, n_H > 1) is not implemented on the GPU");
        g.batch = d->batch; g.H = H; g.M = M; g.K = K; g.N = N;
        g.nVA = nVA; g.nHA = nHA; g.nVB = nVB; g.nHB = nHB;
        g.crA = cdiv(M, nVA); g.ccA = cdiv(K, nHA); g.crB = cdiv(K, nVB); g.ccB = cdiv(N, nHB);
        g.A = t.A; g.B = t.B;
        for (int i = 0; i < 4; ++i) { g.a_st[i] = d->a_stride[i]; g.b_st[i] = d->b_stride[i]; }
        g.Aq = 1 << (d->A_bit - 1); g.Bq = 1 << (d->B_bit - 1); g.sos = d->sos != 0;
        g.ivA = t.A_iv; g.ivB = t.B_iv; g.split = t.split;
        CHK(seg_cut_k(g, "matmul"));
        nA = d->sos ? 1 : H * nVA * nHA; nB = H * nVB * nHB; ncand = d->eq_n + 1;
        const int steps = (d->sos ? 1 : nVA * nHA) + nVB * nHB;
        rounds = SearchRounds(sg, d->search_round, !(d->reserved & RSV_NO_MEMO), d->eq_n, H, c, t.scores, t.best, steps);
        return 0;
    }
    int workspace() {
        enc_A = c.ws.get<unsigned>((size_t)H * nVA * nHA);
        enc_B = c.ws.get<unsigned>((size_t)nB);
        A_cands_ws = c.ws.get<float>((size_t)ncand * H * nVA * nHA);
        B_cands_ws = c.ws.get<float>((size_t)ncand * nB);
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small");
        return 0;
    }
    // min-max per block (a block of nothing but padding gets the interval 0), the intervals, their candidate tables
    int init() {
        if (!sg.inits()) return 0;
        const long sa[4] = {d->a_stride[0], d->a_stride[1], d->a_stride[2], d->a_stride[3]};
        const long sb[4] = {d->b_stride[0], d->b_stride[1], d->b_stride[2], d->b_stride[3]};
        if (!d->sos) {
            CHK(launch_absmax(c, t.A, sa, d->batch, H, M, K, nVA, nHA, g.crA, g.ccA, 0, enc_A, true));
            CHK(launch_interval(c, enc_A, nA, (float)(g.Aq - 0.5), d->init_layerwise, t.A_iv));
        }
        CHK(launch_absmax(c, t.B, sb, d->batch, H, K, N, nVB, nHB, g.crB, g.ccB, 0, enc_B, true));
        CHK(launch_interval(c, enc_B, nB, (float)(g.Bq - 0.5), d->init_layerwise, t.B_iv));
        if (sg.searches()) {
            if (!d->sos) CHK(launch_cands(c, t.mult, t.A_iv, ncand, nA, A_cands_ws));
            CHK(launch_cands(c, t.mult, t.B_iv, ncand, nB, B_cands_ws));
        }
        return 0;
    }
    // quant_forward (matmul.py:140-145; sos: 595-598): intervals / split are inputs
    Pass forward_pass() {
        Pass fp{};
        fp.seg = &g; fp.Z = Z; fp.K = K; fp.Mrows = M; fp.Ncols = N; fp.i8 = true; fp.twin = g.sos;
        fp.epi = EPI_FWD; fp.eq_n = 1; fp.store_out = t.fwd_out;
        return fp;
    }
    // The pass of one block step: `side` 1 / 2 = A / B, candidates cands[c * cs + head * hs] replacing the scale of block (v, h),
    // every other block on the interval entering the step.
    Pass step_pass(int side, int v, int h, const float* cands, int cs, int hs, float* scores, int32_t* best) {
        const int nV = side == 1 ? nVA : nVB, nH = side == 1 ? nHA : nHB;
        g.side = side; g.ov_v = v; g.ov_h = h; g.cands = cands; g.cand_cs = cs; g.cand_hs = hs;     // the plan's override: this block
        Pass ps{};
        ps.seg = &g; ps.Z = Z; ps.K = K; ps.Mrows = M; ps.Ncols = N; ps.i8 = true; ps.twin = g.sos;
        ps.epi = epi; ps.wt_mode = wt_mode; ps.O = t.O; ps.G = t.G; ps.eq_n = d->eq_n;
        ps.j_mode = 2; ps.j_div = H; ps.nj = H; ps.norm = 1.0 / ((double)M * N);
        ps.cands = cands; ps.cand_cs = cs; ps.cand_js = hs; ps.cand_off = 0;
        ps.interval = (side == 1 ? t.A_iv : t.B_iv) + v * nH + h; ps.out_js = nV * nH; ps.out_off = 0;
        ps.scores_out = scores; ps.scores_out_ld = H; ps.best_out = best;
        return ps;
    }
    // granular: ONE block step on the caller's candidate table [eq_n + 1][heads]
    int granular_step(int side, const float* cands) {
        const int nV = side == 1 ? nVA : nVB, nH = side == 1 ? nHA : nHB;
        if (mb.v < 0 || mb.v >= nV || mb.h < 0 || mb.h >= nH) return fail(P4V_ERR_INVALID, "matmul: block (%d, %d) outside the %d x %d blocks", mb.v, mb.h, nV, nH);
        Pass ps = step_pass(side, mb.v, mb.h, cands, H, 1, t.scores, t.best);
        return run_pass(c, ps);
    }
    // the steps of a round: the A blocks (sos: the split search), then the B blocks, each in product(range(n_V), range(n_H)) order
    std::vector<Step> steps(int round) const {
        std::vector<Step> st;
        auto add = [&](int side, int v, int h) { const int s = (int)st.size(); st.push_back({side, v, h, rounds.scores_of(round, s), rounds.best_of(round, s)}); };
        if (d->sos) add(0, 0, 0);
        else for (int v = 0; v < nVA; ++v) for (int h = 0; h < nHA; ++h) add(1, v, h);
        for (int v = 0; v < nVB; ++v) for (int h = 0; h < nHB; ++h) add(2, v, h);
        return st;
    }
    // The split search against the UNQUANTISED B (matmul.py:600-631) knows no blocks: the head-wise engine's pass, as a head-wise
    // call in mode ST_S1 would make it.  A call of its own every round, as it always was: its tables, the split candidates and
    // the slice cache start anew, and its workspace is given back at the end of the step.
    int split_step(const Step& s) {
        const ArenaMark mark(c.ws);
        MatMulCall m(c, d, {.A = t.A, .B = t.B, .O = t.O, .G = t.G, .A_iv = t.A_iv, .split = t.split, .scores = s.scores, .best = s.best}, split_stage);
        m.build();
        CHK(q_wait_inputs(c));
        CHK(m.workspace());
        CHK(m.upload_splits());
        return m.side_passes(0, 0);
    }
    int run_step(const Step& s) {
        if (s.side == 0) return split_step(s);
        const int nV = s.side == 1 ? nVA : nVB, nH = s.side == 1 ? nHA : nHB;
        Pass ps = step_pass(s.side, s.v, s.h, (s.side == 1 ? A_cands_ws : B_cands_ws) + s.v * nH + s.h, H * nV * nH, nV * nH, s.scores, s.best);
        return run_pass(c, ps);
    }
    // The call with sub-blocks, after matmul_impl's checks and its wait for the inputs.  The rounds are a plain loop over the
    // steps: no side has a memo, and a round has more than two steps (search_rounds drives two memoised sides).
    int run() {
        CHK(build());
        CHK(workspace());
        if (sg.forward()) { Pass fp = forward_pass(); return run_pass(c, fp); }
        CHK(init());
        if (!sg.searches()) return 0;
        if (!sg.full()) {
            if (sg.mask & ST_S1) CHK(granular_step(1, sg.cands1));
            if (sg.mask & ST_S2) CHK(granular_step(2, sg.cands2));
            return 0;
        }
        for (int round = 0; round < rounds.n_rounds; ++round)
            for (const Step& s : steps(round)) CHK(run_step(s));
        return 0;
    }
};

int matmul_impl(const p4v_matmul_desc* d, const MatMulTensors& t, const Stage& sg, Ctx& c, const MatMulBlocks& mb = MatMulBlocks{}) {
    CHK(matmul_check(d, t, sg, c));     // (with sub-blocks too: before the checks of the block counts)
    cvt_bias(c);     // (first call of the process: probe the conversion quant16_sat8 relies on)
    CHK(q_wait_inputs(c));     // (inside a group with a "capture done" event: everything below reads captured tensors)
    // row / column sub-blocks: the K-segmented kernel family; with all four block counts 1 the head-wise engine
    if (mb.any()) return MatMulBlocksCall(c, d, mb, t, sg).run();
    return MatMulCall(c, d, t, sg).run();
}

// ------------------------------------------------------------------------------------------------
// Conv2d (patch embedding): fp32 operands (the input stays unquantised with a_bit >= 32, conv.py:544)
// ------------------------------------------------------------------------------------------------
// The device pointers of one conv_impl call are a Linear's: weight [oc][ic][kh][kw], bias [oc], x [b][ic][H][W], raw_out / raw_grad
// [b][oc][fh][fw], intervals [oc] or [1] / [1].  There is no conv forward: fwd_out stays null.
typedef LinearTensors ConvTensors;
// One conv_impl call: what build() derives from the descriptor, and the builders of its passes.  Sides: 0 = the weight search
// (conv.py:526-557 / 365-396), 1 = the activation search (conv.py:559-589; the channel-wise class only).
struct ConvCall {
    Ctx& c;
    const p4v_conv_desc* d;
    const ConvTensors t;
    const Stage& sg;
    int b = 0, ic = 0, H = 0, Wd = 0, oc = 0, kh = 0, kw = 0;  // batch, input channels, image, output channels, kernel
    int fh = 0, fw = 0;                               // output pixels per column / per row
    int L = 0, K = 0, M = 0;                          // pixels of one output image, the im2col row ic x kh x kw, rows: batch x L
    int nw = 1;                                       // weight intervals: one per output channel, or one
    int wq = 0, aq = 0;                               // 2^(bit - 1) of the weights / the input (0: unquantised)
    bool aquant = false;                              // a_bit < 32: the input is quantised and searched
    int epi = 0, wt_mode = 0, ncand = 0;              // the metric's epilogue and weighting, rows of a candidate table
    bool cosm = false;                                // cosine metric
    bool prunable = false;                            // the weight search may be pruned like a Linear's (transpose_targets)
    unsigned *enc_w = nullptr, *enc_a = nullptr;      // abs-max per interval, order-preserving encoding
    float *w_cands_ws = nullptr, *a_cands_ws = nullptr;       // candidate tables built by this call ...
    const float *w_cands = nullptr, *a_cands = nullptr;       // ... or the caller's (granular search)
    float *Ot = nullptr, *Gt = nullptr;               // prunable: raw_out / raw_grad as rows of the im2col GEMM, [b * L][oc]
    SearchRounds rounds;
    PlaneCache plane_w, plane_a;                      // per side: the candidate-expanded plane, kept across rounds
    SliceCache slice;                                 // the row slices of the pruned weight passes

    ConvCall(Ctx& c_, const p4v_conv_desc* d_, const ConvTensors& t_, const Stage& sg_) : c(c_), d(d_), t(grad_by_metric(t_, d_->metric)), sg(sg_) {}

    // argument checks, geometry, the tables' workspace
    int build() {
        b = d->batch; ic = d->in_channels; H = d->height; Wd = d->width; oc = d->out_channels; kh = d->kernel_h; kw = d->kernel_w;
        if (kh <= 0 || kw <= 0 || d->stride_h <= 0 || d->stride_w <= 0 || d->pad_h < 0 || d->pad_w < 0 || d->dil_h <= 0 || d->dil_w <= 0)
            return fail(P4V_ERR_INVALID, "conv: bad geometry");
        // output size floor((size + 2 pad - dil (k - 1) - 1) / stride) + 1: the numerators are tested for their sign -- C division
        // truncates toward zero, so a dilated kernel one larger than the padded image (numerator -1) would give 1 with stride >= 2
        const int num_h = H + 2 * d->pad_h - d->dil_h * (kh - 1) - 1, num_w = Wd + 2 * d->pad_w - d->dil_w * (kw - 1) - 1;
        if (b <= 0 || ic <= 0 || oc <= 0 || H <= 0 || Wd <= 0 || num_h < 0 || num_w < 0 || d->eq_n <= 0) return fail(P4V_ERR_INVALID, "conv: bad geometry");
        fh = num_h / d->stride_h + 1; fw = num_w / d->stride_w + 1;
        if (d->w_bit > 8 || d->w_bit < 2) return fail(P4V_ERR_UNSUPPORTED, "conv: w_bit 2..8 supported");
        if (d->a_bit < 2) return fail(P4V_ERR_UNSUPPORTED, "conv: a_bit >= 2 supported (>= 32: unquantised input)");
        L = fh * fw; K = ic * kh * kw; M = b * L;
        wq = 1 << (d->w_bit - 1);
        aquant = d->a_bit < 32;
        aq = aquant ? (1 << (d->a_bit - 1)) : 0;
        if (aquant && !d->channelwise) return fail(P4V_ERR_UNSUPPORTED, "conv: the layer-wise class cannot search activations (reference conv.py:420 raises IndexError); use a_bit=32");
        cvt_bias(c);     // (first call of the process: probe the conversion quant16_sat8 relies on)
        metric_epi(d->metric, &epi, &wt_mode);
        cosm = epi == EPI_COS;
        if (wt_mode == 1 && !t.G && sg.searches() && !c.dry) return fail(P4V_ERR_INVALID, "conv: hessian metric needs raw_grad");
        if (cosm && aquant) return fail(P4V_ERR_UNSUPPORTED, "conv: cosine does not support the activation search (reference conv.py:505-506)");
        nw = d->channelwise ? oc : 1;
        ncand = d->eq_n + 1;
        rounds = SearchRounds(sg, d->search_round, !(d->reserved & RSV_NO_MEMO), d->eq_n, nw, c, t.scores, t.best);
        enc_w = c.ws.get<unsigned>(nw);
        enc_a = c.ws.get<unsigned>(1);
        w_cands_ws = c.ws.get<float>((size_t)ncand * nw);
        a_cands_ws = c.ws.get<float>(ncand);
        w_cands = sg.inits() ? w_cands_ws : sg.cands1;
        a_cands = sg.inits() ? a_cands_ws : sg.cands2;
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small");
        return 0;
    }
    // interval initialisation of both operands and their candidate tables
    int init() {
        if (!sg.inits()) return 0;
        const long stw[4] = {0, 0, K, 1};
        CHK(launch_absmax(c, t.W, stw, 1, 1, oc, K, nw, 1, d->channelwise ? 1 : oc, K, 0, enc_w));
        CHK(launch_interval(c, enc_w, nw, (float)(wq - 0.5), d->init_layerwise, t.w_iv));
        const long stx[4] = {0, 0, (long)ic * H * Wd, 1};
        CHK(launch_absmax(c, t.X, stx, 1, 1, b, ic * H * Wd, 1, 1, b, ic * H * Wd, 0, enc_a));
        CHK(launch_interval(c, enc_a, 1, aquant ? (float)(aq - 0.5) : (float)(std::ldexp(1.0, d->a_bit - 1) - 0.5), 0, t.a_iv));
        if (sg.searches()) {
            CHK(launch_cands(c, t.mult, t.w_iv, ncand, nw, w_cands_ws));
            CHK(launch_cands(c, t.mult, t.a_iv, ncand, 1, a_cands_ws));
        }
        return 0;
    }
    // The difference metrics read raw_out / raw_grad as rows of the im2col GEMM, [b * L][oc]: one transposition of the [b][oc][L]
    // tensors (same elements, same sums) gives the sweeps a dense epilogue operand and lets the weight search be pruned like a
    // Linear's (run_pass_pruned: slices are rows).
    int transpose_targets() {
        prunable = !cosm && sg.full() && !t.scores && !t.best && !(d->reserved & RSV_NO_PRUNE) && d->eq_n >= 32;
        Ot = prunable ? c.ws.get<float>((size_t)M * oc) : nullptr;
        Gt = (prunable && (t.G || c.dry)) ? c.ws.get<float>((size_t)M * oc) : nullptr;   // (the sizing run plans for a call with raw_grad)
        if (!c.ws.ok()) return fail(P4V_ERR_WORKSPACE, "workspace too small");
        if (!prunable || c.dry) return 0;
        const dim3 grid(cdiv(L, 32), cdiv(oc, 32), b);
        CHK(enqueue(c, KERN(NchwRowsParams, k_nchw_to_rows), grid, dim3(256), 0, NchwRowsParams{t.O, oc, L, Ot}));
        if (t.G) CHK(enqueue(c, KERN(NchwRowsParams, k_nchw_to_rows), grid, dim3(256), 0, NchwRowsParams{t.G, oc, L, Gt}));
        return 0;
    }

    // x as im2col rows.  per_image: Z = batch, rows = pixels of one image (channel-wise cosine reduces over pixels)
    Operand x_operand(bool expanded, const float* scales, int sc_cs, bool per_image) const {
        Operand op{};
        op.present = true; op.expanded = expanded;
        op.pk = PackParams{};
        op.pk.src = t.X; op.pk.conv = 1; op.pk.ic = ic; op.pk.H = H; op.pk.W = Wd; op.pk.kh = kh; op.pk.kw = kw;
        op.pk.sh = d->stride_h; op.pk.sw = d->stride_w; op.pk.ph = d->pad_h; op.pk.pw = d->pad_w; op.pk.dh = d->dil_h; op.pk.dw = d->dil_w;
        op.pk.fw = fw; op.pk.L = L;
        op.pk.Z = per_image ? b : 1; op.pk.s_z = per_image ? (long)ic * H * Wd : 0;
        op.pk.R = per_image ? L : M; op.pk.K = K; op.pk.nblk_r = 1; op.pk.nblk_k = 1;
        op.pk.mode = aquant ? PACK_SYM : PACK_RAW; op.pk.scales = aquant ? scales : nullptr; op.pk.sc_cs = sc_cs;
        op.pk.lo = -aq; op.pk.hi = aq - 1;
        return op;
    }
    Operand w_operand(bool expanded, const float* scales, int sc_cs) const {
        Operand op{};
        op.present = true; op.expanded = expanded;
        op.pk = pack2d(t.W, oc, K, K);
        op.pk.scales = scales; op.pk.sc_cs = sc_cs;
        op.pk.blk_mode = d->channelwise ? 1 : 0; op.pk.blk_div = 1; op.pk.nblk_r = nw; op.pk.nblk_k = 1;
        op.pk.lo = -wq; op.pk.hi = wq - 1;
        return op;
    }
    // The search pass of one side: the searched operand candidate-expanded, the other at its current interval; the GEMM in the
    // orientation of the metric, then the side's selection.
    Pass search_pass(int side, int round) {
        const bool ws = side == 0;
        Pass ps{};
        ps.i8 = false; ps.twin = false; ps.epi = epi; ps.wt_mode = wt_mode; ps.eq_n = d->eq_n; ps.K = K;
        ps.use_s1 = false; ps.s_cs = 1; ps.sb_mode = 0;
        ps.O = t.O; ps.G = t.G; ps.bias = t.bias;
        const Operand xo = x_operand(!ws, ws ? t.a_iv : a_cands, ws ? 0 : 1, cosm && d->channelwise);
        const Operand wo = w_operand(ws, ws ? w_cands : t.w_iv, ws ? nw : 0);
        if (!cosm) {
            // rows = (image, pixel), cols = oc;  out[b][oc][l]
            ps.Z = 1; ps.Mrows = M; ps.Ncols = oc; ps.row = xo; ps.col = wo;
            ps.o_inner = L; ps.o_bs = (long)oc * L; ps.o_ms = 1; ps.o_ns = L; ps.bias_axis = 0;
            if (prunable) { ps.O = Ot; ps.G = t.G ? Gt : nullptr; ps.o_inner = INT_MAX; ps.o_bs = 0; ps.o_ms = oc; ps.o_ns = 1; }
        } else if (d->channelwise) {
            // cosine over the pixels of one image per (image, oc) (conv.py:504-508): rows = pixels, z = image
            ps.Z = b; ps.Mrows = L; ps.Ncols = oc; ps.row = xo; ps.col = wo; ps.col_zs_shared = 1;
            ps.o_zs = (long)oc * L; ps.o_inner = INT_MAX; ps.o_ms = 1; ps.o_ns = L; ps.bias_axis = 0; ps.G = nullptr;
            ps.cos_ZB = b; ps.cos_ZV = 1;
        } else {
            // cosine over oc per pixel (conv.py:387): swapped, rows = oc, cols = (image, pixel)
            ps.Z = 1; ps.Mrows = oc; ps.Ncols = M; ps.row = wo; ps.col = xo;
            // element (row=oc, col=m): idx = (m / L)*oc*L + (m % L) + oc_idx*L  -> column index drives the image split
            ps.o_inner = INT_MAX; ps.o_ms = L; ps.o_ninner = L; ps.o_nbs = (long)oc * L; ps.o_ns = 1;
            ps.bias_axis = 1; ps.G = nullptr;
            ps.cos_ZB = 1; ps.cos_ZV = 1;
        }
        if (ws) {   // one score column and one interval per weight interval
            ps.nj = nw;
            if (!cosm) { ps.j_mode = d->channelwise ? 3 : 0; ps.norm = d->channelwise ? 1.0 / (double)L : 1.0 / ((double)L * oc); }
            else if (d->channelwise) { ps.cos_j_mode = 3; ps.norm = 1.0; }
            else { ps.cos_j_mode = 0; ps.norm = 1.0 / (double)L; }
            ps.cands = w_cands; ps.cand_cs = nw; ps.cand_js = 1; ps.interval = t.w_iv; ps.out_js = 1;
            ps.prunable = ps.prunable_f32 = prunable; ps.scache = &slice; ps.host_sync_ok = rounds.memo_on;
        } else {    // the one interval of the input
            ps.nj = 1; ps.j_mode = 0; ps.norm = 1.0 / ((double)L * oc);
            ps.cands = a_cands; ps.cand_cs = 1; ps.cand_js = 0; ps.interval = t.a_iv; ps.out_js = 0;
        }
        ps.cache = rounds.keep_planes ? (ws ? &plane_w : &plane_a) : nullptr;
        ps.scores_out = rounds.scores_of(round, side); ps.scores_out_ld = nw; ps.best_out = rounds.best_of(round, side);
        return ps;
    }
    // The weight side may be pruned; with a_bit >= 32 the input is never quantised: the weight search depends on nothing
    // (conv.py:544), and there is no activation side -- no Stage bit, no memo.
    SearchSide search_side(int side) {
        const DevVecs w(t.w_iv, nw), a(t.a_iv, 1);
        if (side == 0)
            return SearchSide(ST_S1, rounds.memo_on, aquant ? a : DevVecs(), w, [this](int round) { Pass ps = search_pass(0, round); return run_pass_pruned(c, ps); });
        return SearchSide(aquant ? ST_S2 : 0, rounds.memo_on && aquant, w, a, [this](int round) { Pass ps = search_pass(1, round); return run_pass(c, ps); });
    }
};

int conv_impl(const p4v_conv_desc* d, const ConvTensors& t, const Stage& sg, Ctx& c) {
    ConvCall cv(c, d, t, sg);
    CHK(cv.build());
    CHK(q_wait_inputs(c));     // (inside a group with a "capture done" event: everything below reads captured tensors)
    CHK(cv.init());
    if (!sg.searches()) return 0;
    CHK(cv.transpose_targets());
    MirrorScope mirrors(c, cv.rounds.memo_on, t.w_iv, t.a_iv);
    SearchSide sides[2] = {cv.search_side(0), cv.search_side(1)};
    return search_rounds(c, cv.rounds, sg, sides, nullptr);
}

// ---- p4v_calibrate_group: the members' calibration_step2 in lock step, launches grouped ----------------------------------------
// Worker threads are persistent (a ViT-B calibration runs 74 members; thread creation per call would cost as much as a search
// pass): a task is handed to an idle worker or a new one is started -- every member of a group must be running at the same time,
// they rendezvous.  The pool object is never destroyed (workers are detached and outlive static destruction order).
struct WorkerPool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> tasks;
    int idle = 0;
    void run(std::function<void()> f) {
        std::unique_lock<std::mutex> lk(mu);
        tasks.push_back(std::move(f));
        if (idle >= (int)tasks.size()) { cv.notify_one(); return; }
        lk.unlock();
        std::thread([this] { loop(); }).detach();
    }
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            while (tasks.empty()) { ++idle; cv.wait(lk); --idle; }
            auto f = std::move(tasks.front());
            tasks.pop_front();
            lk.unlock();
            f();
            lk.lock();
        }
    }
};
WorkerPool& worker_pool() { static WorkerPool* p = new WorkerPool; return *p; }

int* group_mirror(hipStream_t st, int dev, int slot) {
    static std::mutex mu;
    static std::unordered_map<std::string, int*> tab;
    char key[64];
    snprintf(key, sizeof key, "%p/%d/%d", (void*)st, dev, slot);
    std::lock_guard<std::mutex> lk(mu);
    auto it = tab.find(key);
    if (it != tab.end()) return it->second;
    int* p = mirror_alloc();
    tab[key] = p;
    return p;
}

// one member = one p4v_*_calibrate call without tables: in = {weight, bias, x, raw_out, raw_grad} (MatMul: {A, B, raw_out, raw_grad})
int run_group_member(const p4v_group_job& j, Ctx& c) {
    switch (j.kind) {
        case P4V_JOB_LINEAR: {
            const p4v_linear_desc* d = (const p4v_linear_desc*)j.desc;
            if (!j.in[0] || !j.in[2] || !j.in[3] || !j.mult || !j.out[0] || !j.out[1] || !j.workspace) return fail(P4V_ERR_INVALID, "group: linear member with a null pointer");
            if (d->has_bias && !j.in[1]) return fail(P4V_ERR_INVALID, "group: linear member has_bias set but bias is NULL");
            return linear_impl(d, {.W = j.in[0], .bias = d->has_bias ? j.in[1] : nullptr, .X = j.in[2], .O = j.in[3], .G = j.in[4], .mult = j.mult,
                                   .w_iv = j.out[0], .a_iv = j.out[1]}, Stage{}, c);
        }
        case P4V_JOB_MATMUL: case P4V_JOB_MATMUL_BLOCKS: {
            const p4v_matmul_blocks_desc* bd = j.kind == P4V_JOB_MATMUL_BLOCKS ? (const p4v_matmul_blocks_desc*)j.desc : nullptr;
            const p4v_matmul_desc* d = bd ? &bd->mm : (const p4v_matmul_desc*)j.desc;
            if (!j.in[0] || !j.in[1] || !j.in[2] || !j.mult || !j.out[0] || !j.out[1] || !j.workspace) return fail(P4V_ERR_INVALID, "group: matmul member with a null pointer");
            if (bd) CHK(blocks_check(bd, "group", "matmul member with a "));
            return matmul_impl(d, {.A = j.in[0], .B = j.in[1], .O = j.in[2], .G = j.in[3], .mult = j.mult, .A_iv = j.out[0], .B_iv = j.out[1],
                                   .split = j.out[2]}, Stage{}, c, bd ? blocks_of(bd) : MatMulBlocks{});
        }
        case P4V_JOB_CONV: {
            const p4v_conv_desc* d = (const p4v_conv_desc*)j.desc;
            if (!j.in[0] || !j.in[2] || !j.in[3] || !j.mult || !j.out[0] || !j.out[1] || !j.workspace) return fail(P4V_ERR_INVALID, "group: conv member with a null pointer");
            if (d->has_bias && !j.in[1]) return fail(P4V_ERR_INVALID, "group: conv member has_bias set but bias is NULL");
            return conv_impl(d, {.W = j.in[0], .bias = d->has_bias ? j.in[1] : nullptr, .X = j.in[2], .O = j.in[3], .G = j.in[4], .mult = j.mult,
                                 .w_iv = j.out[0], .a_iv = j.out[1]}, Stage{}, c);
        }
        default: return fail(P4V_ERR_INVALID, "group: unknown member kind %d", j.kind);
    }
}
size_t group_desc_bytes(int kind) {
    return kind == P4V_JOB_LINEAR ? sizeof(p4v_linear_desc) : kind == P4V_JOB_MATMUL ? sizeof(p4v_matmul_desc) : kind == P4V_JOB_CONV ? sizeof(p4v_conv_desc) :
           kind == P4V_JOB_MATMUL_BLOCKS ? sizeof(p4v_matmul_blocks_desc) : 0;
}

}  // namespace

// =================================================================================================
extern "C" {

int p4v_version(void) { return P4V_VERSION; }
const char* p4v_last_error(void) { return g_err.c_str(); }

// The prologue of the entry points whose checks are only these, in this order: the required pointers, the bias the descriptor
// announces, the workspace's alignment.  (The MatMul entry points and conv_search have checks of their own in between.)
static int entry_checks(const char* who, bool present, bool bias_missing, const void* d_workspace, const char* bias_null = "d_bias is NULL") {
    if (!present || !d_workspace) return fail(P4V_ERR_INVALID, "%s: null pointer", who);
    if (bias_missing) return fail(P4V_ERR_INVALID, "%s: has_bias set but %s", who, bias_null);
    return ws_aligned(d_workspace);
}

size_t p4v_linear_workspace_bytes(const p4v_linear_desc* desc) {
    if (!desc) return 0;
    Ctx c = Ctx::sizing();
    return linear_impl(desc, LinearTensors{}, sizing_stage(desc->reserved), c) == 0 ? c.sized_bytes() : 0;
}

int p4v_linear_calibrate(const p4v_linear_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                         const float* d_out, const float* d_grad, const float* d_mult, float* d_w_interval,
                         float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
    CHK(entry_checks("linear", desc && d_weight && d_x && d_out && d_mult && d_w_interval && d_a_interval, desc && desc->has_bias && !d_bias, d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return linear_impl(desc, {.W = d_weight, .bias = desc->has_bias ? d_bias : nullptr, .X = d_x, .O = d_out, .G = d_grad, .mult = d_mult,
                              .w_iv = d_w_interval, .a_iv = d_a_interval, .scores = d_scores, .best = d_best}, Stage{}, c);
}

int p4v_linear_quant_forward(const p4v_linear_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                             const float* d_w_interval, const float* d_a_interval, float* d_out, void* d_workspace,
                             size_t workspace_bytes, void* stream) {
    CHK(entry_checks("p4v_linear_quant_forward", desc && d_weight && d_x && d_w_interval && d_a_interval && d_out, desc && desc->has_bias && !d_bias,
                     d_workspace, "d_bias is null"));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return linear_impl(desc, {.W = d_weight, .bias = desc->has_bias ? d_bias : nullptr, .X = d_x, .w_iv = const_cast<float*>(d_w_interval),
                              .a_iv = const_cast<float*>(d_a_interval), .fwd_out = d_out}, Stage{ST_FWD}, c);
}

size_t p4v_mlp_workspace_bytes(const p4v_mlp_desc* desc) {
    size_t need = 0;
    return (desc && fused_sizing_run(mlp_impl, desc, &need) == 0) ? need : 0;
}

int p4v_mlp_quant_forward(const p4v_mlp_desc* desc, const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                          const float* d_x, const float* d_w1_interval, const float* d_a1_interval, const float* d_w2_interval,
                          const float* d_a2_interval, float* d_out, float* d_hidden, void* d_ws, size_t ws_bytes, void* stream) {
    CHK(entry_checks("p4v_mlp_quant_forward", desc && d_w1 && d_w2 && d_x && d_w1_interval && d_a1_interval && d_w2_interval && d_a2_interval && d_out,
                     desc && ((desc->fc1.has_bias && !d_b1) || (desc->fc2.has_bias && !d_b2)), d_ws, "the bias is null"));
    return fused_call(mlp_impl, desc,
                      {.W = d_w1, .bias = desc->fc1.has_bias ? d_b1 : nullptr, .X = d_x, .w_iv = const_cast<float*>(d_w1_interval),
                       .a_iv = const_cast<float*>(d_a1_interval), .fwd_out = d_hidden},
                      {.W = d_w2, .bias = desc->fc2.has_bias ? d_b2 : nullptr, .w_iv = const_cast<float*>(d_w2_interval),
                       .a_iv = const_cast<float*>(d_a2_interval), .fwd_out = d_out}, d_ws, ws_bytes, stream);
}

size_t p4v_attn_workspace_bytes(const p4v_attn_desc* desc) {
    size_t need = 0;
    return (desc && fused_sizing_run(attn_impl, desc, &need) == 0) ? need : 0;
}

int p4v_attn_quant_forward(const p4v_attn_desc* desc, const float* d_q, const float* d_kT, const float* d_v,
                           const float* d_qk_A_interval, const float* d_qk_B_interval, const float* d_pv_A_interval,
                           const float* d_pv_B_interval, const float* d_split, float* d_out, float* d_probs, void* d_ws,
                           size_t ws_bytes, void* stream) {
    if (!desc || !d_q || !d_kT || !d_v || !d_qk_A_interval || !d_qk_B_interval || !d_pv_A_interval || !d_pv_B_interval || !d_out || !d_ws)
        return fail(P4V_ERR_INVALID, "p4v_attn_quant_forward: null pointer");
    if (desc->pv.sos && !d_split) return fail(P4V_ERR_INVALID, "p4v_attn_quant_forward: sos needs d_split");
    CHK(ws_aligned(d_ws));
    return fused_call(attn_impl, desc,
                      {.A = d_q, .B = d_kT, .A_iv = const_cast<float*>(d_qk_A_interval), .B_iv = const_cast<float*>(d_qk_B_interval), .fwd_out = d_probs},
                      {.B = d_v, .A_iv = const_cast<float*>(d_pv_A_interval), .B_iv = const_cast<float*>(d_pv_B_interval),
                       .split = const_cast<float*>(d_split), .fwd_out = d_out}, d_ws, ws_bytes, stream);
}

static WattnCall wattn_call(const p4v_wattn_desc* desc, const p4v_wattn_tensors* t) {
    WattnCall w{};
    w.a.qk = desc->qk; w.a.pv = desc->pv; w.a.scale = 1.0f;
    w.w = AttnWindow{t ? t->bias : nullptr, t ? t->mask : nullptr, desc->n_windows};
    return w;
}
size_t p4v_wattn_workspace_bytes(const p4v_wattn_desc* desc) {
    if (!desc) return 0;
    const WattnCall w = wattn_call(desc, nullptr);
    size_t need = 0;
    return fused_sizing_run(wattn_impl, &w, &need) == 0 ? need : 0;
}

int p4v_wattn_quant_forward(const p4v_wattn_desc* desc, const p4v_wattn_tensors* t, void* stream) {
    if (!desc || !t || !t->q || !t->kT || !t->v || !t->bias || !t->qk_A_interval || !t->qk_B_interval || !t->pv_A_interval || !t->pv_B_interval ||
        !t->out || !t->ws)
        return fail(P4V_ERR_INVALID, "p4v_wattn_quant_forward: null pointer");
    if (desc->pv.sos && !t->split) return fail(P4V_ERR_INVALID, "p4v_wattn_quant_forward: sos needs split");
    if ((desc->has_mask != 0) != (t->mask != nullptr))
        return fail(P4V_ERR_INVALID, "p4v_wattn_quant_forward: has_mask = %d but the mask pointer is %s", desc->has_mask, t->mask ? "set" : "null");
    CHK(ws_aligned(t->ws));
    const WattnCall w = wattn_call(desc, t);
    return fused_call(wattn_impl, &w,
                      {.A = t->q, .B = t->kT, .A_iv = const_cast<float*>(t->qk_A_interval), .B_iv = const_cast<float*>(t->qk_B_interval), .fwd_out = t->probs},
                      {.B = t->v, .A_iv = const_cast<float*>(t->pv_A_interval), .B_iv = const_cast<float*>(t->pv_B_interval),
                       .split = const_cast<float*>(t->split), .fwd_out = t->out}, t->ws, t->ws_bytes, stream);
}

size_t p4v_qkv_attn_workspace_bytes(const p4v_qkv_attn_desc* desc) {
    size_t need = 0;
    return (desc && fused_sizing_run(qkv_attn_impl, desc, &need) == 0) ? need : 0;
}

int p4v_qkv_attn_quant_forward(const p4v_qkv_attn_desc* desc, const p4v_qkv_attn_tensors* t, void* stream) {
    if (!desc || !t || !t->x || !t->w || !t->w_interval || !t->a_interval || !t->qk_A_interval || !t->qk_B_interval || !t->pv_A_interval ||
        !t->pv_B_interval || !t->out || !t->ws)
        return fail(P4V_ERR_INVALID, "p4v_qkv_attn_quant_forward: null pointer");
    if (desc->qkv.has_bias && !t->bias) return fail(P4V_ERR_INVALID, "p4v_qkv_attn_quant_forward: has_bias set but the bias is null");
    if (desc->pv.sos && !t->split) return fail(P4V_ERR_INVALID, "p4v_qkv_attn_quant_forward: sos needs split");
    CHK(ws_aligned(t->ws));
    const QkvAttnTensors rec{
        {.W = t->w, .bias = desc->qkv.has_bias ? t->bias : nullptr, .X = t->x, .w_iv = const_cast<float*>(t->w_interval),
         .a_iv = const_cast<float*>(t->a_interval), .fwd_out = t->qkv_out},
        {.A_iv = const_cast<float*>(t->qk_A_interval), .B_iv = const_cast<float*>(t->qk_B_interval), .fwd_out = t->probs},
        {.A_iv = const_cast<float*>(t->pv_A_interval), .B_iv = const_cast<float*>(t->pv_B_interval), .split = const_cast<float*>(t->split), .fwd_out = t->out}};
    return fused_call(qkv_attn_impl, desc, rec, rec, t->ws, t->ws_bytes, stream);
}

int p4v_matmul_quant_forward(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_A_interval,
                             const float* d_B_interval, const float* d_split, float* d_out, void* d_workspace,
                             size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_A_interval || !d_B_interval || !d_out || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_quant_forward: null pointer");
    if (desc->sos && !d_split) return fail(P4V_ERR_INVALID, "p4v_matmul_quant_forward: sos needs d_split");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .A_iv = const_cast<float*>(d_A_interval), .B_iv = const_cast<float*>(d_B_interval),
                              .split = const_cast<float*>(d_split), .fwd_out = d_out}, Stage{ST_FWD}, c);
}

size_t p4v_matmul_workspace_bytes(const p4v_matmul_desc* desc) {
    if (!desc) return 0;
    Ctx c = Ctx::sizing();
    return matmul_impl(desc, MatMulTensors{}, sizing_stage(desc->reserved), c) == 0 ? c.sized_bytes() : 0;
}

int p4v_matmul_calibrate(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out,
                         const float* d_grad, const float* d_mult, float* d_A_interval, float* d_B_interval, float* d_split,
                         float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_mult || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "matmul: null pointer");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .mult = d_mult, .A_iv = d_A_interval, .B_iv = d_B_interval,
                              .split = d_split, .scores = d_scores, .best = d_best}, Stage{}, c);
}

// ---- MatMul with row / column sub-blocks: matmul_impl with the block counts (all 1: the head-wise path, launch for launch) ----
size_t p4v_matmul_blocks_workspace_bytes(const p4v_matmul_blocks_desc* desc) {
    if (!desc || blocks_check(desc, "p4v_matmul_blocks_workspace_bytes")) return 0;
    Ctx c = Ctx::sizing();
    return matmul_impl(&desc->mm, MatMulTensors{}, sizing_stage(desc->mm.reserved), c, blocks_of(desc)) == 0 ? c.sized_bytes() : 0;
}

int p4v_matmul_blocks_calibrate(const p4v_matmul_blocks_desc* desc, const float* d_A, const float* d_B, const float* d_out,
                                const float* d_grad, const float* d_mult, float* d_A_interval, float* d_B_interval,
                                float* d_split, float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes,
                                void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_mult || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_calibrate: null pointer");
    CHK(blocks_check(desc, "p4v_matmul_blocks_calibrate"));
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(&desc->mm, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .mult = d_mult, .A_iv = d_A_interval, .B_iv = d_B_interval,
                                   .split = d_split, .scores = d_scores, .best = d_best}, Stage{}, c, blocks_of(desc));
}

int p4v_amax_init_matmul_blocks(const p4v_matmul_blocks_desc* desc, const float* d_A, const float* d_B, float* d_A_interval,
                                float* d_B_interval, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_amax_init_matmul_blocks: null pointer");
    CHK(blocks_check(desc, "p4v_amax_init_matmul_blocks"));
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(&desc->mm, {.A = d_A, .B = d_B, .A_iv = d_A_interval, .B_iv = d_B_interval}, Stage{ST_INIT}, c, blocks_of(desc));
}

int p4v_matmul_blocks_search(const p4v_matmul_blocks_desc* desc, int32_t operand, int32_t v, int32_t h, const float* d_A,
                             const float* d_B, const float* d_out, const float* d_grad, const float* d_cands,
                             float* d_A_interval, float* d_B_interval, const float* d_split, float* d_scores, int32_t* d_best,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_cands || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_search: null pointer");
    CHK(blocks_check(desc, "p4v_matmul_blocks_search"));
    if (operand != 0 && operand != 1) return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_search: operand is 0 (A) or 1 (B)");
    if (operand == 0 && desc->mm.sos) return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_search: the split-of-softmax class searches its split (p4v_sos_search_split)");
    if (desc->mm.sos && !d_split) return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_search: sos needs d_split");
    const int nV = operand == 0 ? desc->n_V_A : desc->n_V_B, nH = operand == 0 ? desc->n_H_A : desc->n_H_B;
    if (v < 0 || v >= nV || h < 0 || h >= nH) return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_search: block (%d, %d) outside the %d x %d blocks", v, h, nV, nH);
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(&desc->mm, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .A_iv = d_A_interval, .B_iv = d_B_interval,
                                   .split = const_cast<float*>(d_split), .scores = d_scores, .best = d_best},
                       operand == 0 ? Stage{ST_S1, d_cands, nullptr} : Stage{ST_S2, nullptr, d_cands}, c, blocks_of(desc, v, h));
}

int p4v_matmul_blocks_quant_forward(const p4v_matmul_blocks_desc* desc, const float* d_A, const float* d_B,
                                    const float* d_A_interval, const float* d_B_interval, const float* d_split, float* d_out,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_A_interval || !d_B_interval || !d_out || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_quant_forward: null pointer");
    CHK(blocks_check(desc, "p4v_matmul_blocks_quant_forward"));
    if (desc->mm.sos && !d_split) return fail(P4V_ERR_INVALID, "p4v_matmul_blocks_quant_forward: sos needs d_split");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(&desc->mm, {.A = d_A, .B = d_B, .A_iv = const_cast<float*>(d_A_interval), .B_iv = const_cast<float*>(d_B_interval),
                                   .split = const_cast<float*>(d_split), .fwd_out = d_out}, Stage{ST_FWD}, c, blocks_of(desc));
}

size_t p4v_conv_workspace_bytes(const p4v_conv_desc* desc) {
    if (!desc) return 0;
    Ctx c = Ctx::sizing();
    return conv_impl(desc, ConvTensors{}, Stage{}, c) == 0 ? c.sized_bytes() : 0;
}

int p4v_conv_calibrate(const p4v_conv_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                       const float* d_out, const float* d_grad, const float* d_mult, float* d_w_interval, float* d_a_interval,
                       float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes, void* stream) {
    CHK(entry_checks("conv", desc && d_weight && d_x && d_out && d_mult && d_w_interval && d_a_interval, desc && desc->has_bias && !d_bias, d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return conv_impl(desc, {.W = d_weight, .bias = desc->has_bias ? d_bias : nullptr, .X = d_x, .O = d_out, .G = d_grad, .mult = d_mult,
                            .w_iv = d_w_interval, .a_iv = d_a_interval, .scores = d_scores, .best = d_best}, Stage{}, c);
}


int p4v_calibrate_group(p4v_group_job* jobs, int32_t n_jobs, void* stream, void* inputs_ready_event) {
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return fail(P4V_ERR_INVALID, "p4v_calibrate_group: bad job list");
    if (n_jobs == 0) return 0;
    for (int i = 0; i < n_jobs; ++i) {
        jobs[i].status = 0;
        if (!jobs[i].desc || group_desc_bytes(jobs[i].kind) == 0) return fail(P4V_ERR_INVALID, "p4v_calibrate_group: member %d has no descriptor / an unknown kind", i);
        if ((uintptr_t)jobs[i].workspace % WS_ALIGN) return fail(P4V_ERR_INVALID, "p4v_calibrate_group: member %d: workspace must be aligned to %zu bytes", i, WS_ALIGN);
    }
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    cvt_probe((hipStream_t)stream);
    Group g;
    g.st = (hipStream_t)stream; g.n = n_jobs;
    g.q.resize(n_jobs); g.state.assign(n_jobs, 0); g.mirrors.resize(n_jobs);
    for (int i = 0; i < n_jobs; ++i) g.mirrors[i] = group_mirror(g.st, dev, i);
    g.stat_on = g_stat_on;
    g.stat_recs = g_stat_on ? &g_stat_recs : nullptr;
    g.inputs_ready = (hipEvent_t)inputs_ready_event;
    g_launch_cnt[3].fetch_add(1, std::memory_order_relaxed);
    std::vector<std::string> errs(n_jobs);
    std::atomic<long> memo_hits{0}, memo_misses{0};
    std::mutex dmu;
    std::condition_variable dcv;
    int left = n_jobs;
    for (int i = 0; i < n_jobs; ++i) {
        // members with the same descriptor run the same launches in lock step: they share the chip
        int par = 0;
        for (int k = 0; k < n_jobs; ++k)
            par += jobs[k].kind == jobs[i].kind && std::memcmp(jobs[k].desc, jobs[i].desc, group_desc_bytes(jobs[i].kind)) == 0;
        worker_pool().run([&, i, par] {
            (void)hipSetDevice(dev);
            g_stat_on = g.stat_on; g_stage = 0; g_exec_frac = 1.0; g_memo_hits = 0; g_memo_misses = 0; g_err.clear();
            Ctx c{g.st, Arena(jobs[i].workspace, jobs[i].workspace_bytes), false, &g, i, par};
            const int r = run_group_member(jobs[i], c);
            jobs[i].status = r;
            if (r) errs[i] = g_err;
            memo_hits += g_memo_hits; memo_misses += g_memo_misses;
            g_stat_on = false;
            g.finish(i);
            std::lock_guard<std::mutex> lk(dmu);
            if (--left == 0) dcv.notify_all();
        });
    }
    {
        std::unique_lock<std::mutex> lk(dmu);
        dcv.wait(lk, [&] { return left == 0; });
    }
    g_memo_hits += memo_hits.load(); g_memo_misses += memo_misses.load();
    if (tune(TUNE_PRINT) > 0) fprintf(stderr, "[p4v] group of %d: %ld launches asked for, %ld issued in %ld rounds\n", n_jobs, g.n_ops, g.n_launches, g.n_rounds);
    if (g.status) { g_err = g.err; return g.status; }
    for (int i = 0; i < n_jobs; ++i)
        if (jobs[i].status) { g_err = errs[i]; return jobs[i].status; }
    return 0;
}

int p4v_launch_counters(int64_t* out4, int reset) {
    if (out4) for (int i = 0; i < 4; ++i) out4[i] = (int64_t)g_launch_cnt[i].load(std::memory_order_relaxed);
    if (reset) for (int i = 0; i < 4; ++i) g_launch_cnt[i].store(0, std::memory_order_relaxed);
    return 0;
}

// ---- granular entry points: one part of calibration_step2 per call ----------
int p4v_amax_init_linear(const p4v_linear_desc* desc, const float* d_weight, const float* d_x, float* d_w_interval,
                         float* d_a_interval, void* d_workspace, size_t workspace_bytes, void* stream) {
    CHK(entry_checks("p4v_amax_init_linear", desc && d_weight && d_x && d_w_interval && d_a_interval, false, d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return linear_impl(desc, {.W = d_weight, .X = d_x, .w_iv = d_w_interval, .a_iv = d_a_interval}, Stage{ST_INIT}, c);
}

// one side's search on the caller's candidate table: `sg` says which
static int linear_search(const char* who, const Stage& sg, const p4v_linear_desc* desc, const float* d_weight, const float* d_bias,
                         const float* d_x, const float* d_out, const float* d_grad, const float* d_w_interval, const float* d_a_interval,
                         float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes, void* stream) {
    CHK(entry_checks(who, desc && d_weight && d_x && d_out && (sg.cands1 || sg.cands2) && d_w_interval && d_a_interval,
                     desc && desc->has_bias && !d_bias, d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return linear_impl(desc, {.W = d_weight, .bias = desc->has_bias ? d_bias : nullptr, .X = d_x, .O = d_out, .G = d_grad,
                              .w_iv = const_cast<float*>(d_w_interval), .a_iv = const_cast<float*>(d_a_interval), .scores = d_scores,
                              .best = d_best}, sg, c);
}

int p4v_linear_search_w(const p4v_linear_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                        const float* d_out, const float* d_grad, const float* d_w_cands, float* d_w_interval,
                        const float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
    return linear_search("p4v_linear_search_w", Stage{ST_S1, d_w_cands, nullptr}, desc, d_weight, d_bias, d_x, d_out, d_grad, d_w_interval,
                         d_a_interval, d_scores, d_best, d_workspace, workspace_bytes, stream);
}

int p4v_linear_search_a(const p4v_linear_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                        const float* d_out, const float* d_grad, const float* d_a_cands, const float* d_w_interval,
                        float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    return linear_search("p4v_linear_search_a", Stage{ST_S2, nullptr, d_a_cands}, desc, d_weight, d_bias, d_x, d_out, d_grad, d_w_interval,
                         d_a_interval, d_scores, d_best, d_workspace, workspace_bytes, stream);
}

int p4v_amax_init_matmul(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, float* d_A_interval,
                         float* d_B_interval, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_amax_init_matmul: null pointer");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .A_iv = d_A_interval, .B_iv = d_B_interval}, Stage{ST_INIT}, c);
}

int p4v_matmul_search_A(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out,
                        const float* d_grad, const float* d_A_cands, float* d_A_interval, const float* d_B_interval,
                        float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_A_cands || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_search_A: null pointer");
    if (desc->sos) return fail(P4V_ERR_INVALID, "p4v_matmul_search_A: the split-of-softmax class searches its split (p4v_sos_search_split)");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .A_iv = d_A_interval, .B_iv = const_cast<float*>(d_B_interval),
                              .scores = d_scores, .best = d_best}, Stage{ST_S1, d_A_cands, nullptr}, c);
}

int p4v_sos_search_split(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out,
                         const float* d_grad, float* d_split, float* d_A_interval, float* d_scores, int32_t* d_best,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_split || !d_A_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_sos_search_split: null pointer");
    if (!desc->sos) return fail(P4V_ERR_INVALID, "p4v_sos_search_split: descriptor is not a split-of-softmax matmul");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .A_iv = d_A_interval, .split = d_split, .scores = d_scores,
                              .best = d_best}, Stage{ST_S1}, c);
}

int p4v_matmul_search_B(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out,
                        const float* d_grad, const float* d_B_cands, const float* d_A_interval, const float* d_split,
                        float* d_B_interval, float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_B_cands || !d_A_interval || !d_B_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "p4v_matmul_search_B: null pointer");
    if (desc->sos && !d_split) return fail(P4V_ERR_INVALID, "p4v_matmul_search_B: sos needs d_split");
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return matmul_impl(desc, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .A_iv = const_cast<float*>(d_A_interval), .B_iv = d_B_interval,
                              .split = const_cast<float*>(d_split), .scores = d_scores, .best = d_best}, Stage{ST_S2, nullptr, d_B_cands}, c);
}

int p4v_amax_init_conv(const p4v_conv_desc* desc, const float* d_weight, const float* d_x, float* d_w_interval,
                       float* d_a_interval, void* d_workspace, size_t workspace_bytes, void* stream) {
    CHK(entry_checks("p4v_amax_init_conv", desc && d_weight && d_x && d_w_interval && d_a_interval, false, d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return conv_impl(desc, {.W = d_weight, .X = d_x, .w_iv = d_w_interval, .a_iv = d_a_interval}, Stage{ST_INIT}, c);
}

static int conv_search(const char* who, int want_channelwise, int stage, const p4v_conv_desc* desc, const float* d_weight,
                       const float* d_bias, const float* d_x, const float* d_out, const float* d_grad, const float* d_cands,
                       float* d_w_interval, float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
    if (!desc || !d_weight || !d_x || !d_out || !d_cands || !d_w_interval || !d_a_interval || !d_workspace)
        return fail(P4V_ERR_INVALID, "%s: null pointer", who);
    if (desc->has_bias && !d_bias) return fail(P4V_ERR_INVALID, "%s: has_bias set but d_bias is NULL", who);
    if (want_channelwise >= 0 && (desc->channelwise != 0) != (want_channelwise != 0))
        return fail(P4V_ERR_INVALID, "%s: descriptor.channelwise does not match the entry point", who);
    CHK(ws_aligned(d_workspace));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    return conv_impl(desc, {.W = d_weight, .bias = desc->has_bias ? d_bias : nullptr, .X = d_x, .O = d_out, .G = d_grad, .w_iv = d_w_interval,
                            .a_iv = d_a_interval, .scores = d_scores, .best = d_best},
                     stage == ST_S1 ? Stage{ST_S1, d_cands, nullptr} : Stage{ST_S2, nullptr, d_cands}, c);
}

int p4v_conv_search_w_channelwise(const p4v_conv_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                                  const float* d_out, const float* d_grad, const float* d_w_cands, float* d_w_interval,
                                  const float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace,
                                  size_t workspace_bytes, void* stream) {
    return conv_search("p4v_conv_search_w_channelwise", 1, ST_S1, desc, d_weight, d_bias, d_x, d_out, d_grad, d_w_cands,
                       d_w_interval, const_cast<float*>(d_a_interval), d_scores, d_best, d_workspace, workspace_bytes, stream);
}

int p4v_conv_search_w_layerwise(const p4v_conv_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                                const float* d_out, const float* d_grad, const float* d_w_cands, float* d_w_interval,
                                const float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    return conv_search("p4v_conv_search_w_layerwise", 0, ST_S1, desc, d_weight, d_bias, d_x, d_out, d_grad, d_w_cands,
                       d_w_interval, const_cast<float*>(d_a_interval), d_scores, d_best, d_workspace, workspace_bytes, stream);
}

int p4v_conv_search_a(const p4v_conv_desc* desc, const float* d_weight, const float* d_bias, const float* d_x,
                      const float* d_out, const float* d_grad, const float* d_a_cands, const float* d_w_interval,
                      float* d_a_interval, float* d_scores, int32_t* d_best, void* d_workspace, size_t workspace_bytes,
                      void* stream) {
    if (desc && desc->a_bit >= 32) return fail(P4V_ERR_INVALID, "p4v_conv_search_a: a_bit >= 32 leaves the input unquantised (conv.py:600)");
    return conv_search("p4v_conv_search_a", -1, ST_S2, desc, d_weight, d_bias, d_x, d_out, d_grad, d_a_cands,
                       const_cast<float*>(d_w_interval), d_a_interval, d_scores, d_best, d_workspace, workspace_bytes, stream);
}

int p4v_score_argmax_gather(const float* d_scores, int32_t eq_n, int32_t n_blocks, const float* d_cands, float* d_interval,
                            int32_t* d_best, void* stream) {
    if (!d_scores || !d_cands || !d_interval || eq_n <= 0 || n_blocks <= 0)
        return fail(P4V_ERR_INVALID, "p4v_score_argmax_gather: bad argument");
    Ctx c = Ctx::on(stream, nullptr, 0);
    SelectParams sl{d_scores, eq_n, n_blocks, d_cands, n_blocks, 1, 0, d_interval, 1, 0, nullptr, 0.0f, nullptr, 0, d_best};
    return launch_select(c, sl);
}

int p4v_quantize_i8(const float* d_x, int64_t rows, int64_t cols, int64_t cols_padded, const float* d_scales,
                    int64_t rows_per_scale, int32_t lo, int32_t hi, int8_t* d_q, void* stream) {
    if (!d_x || !d_scales || !d_q || rows <= 0 || cols <= 0 || cols_padded % 64 || cols_padded < cols || rows_per_scale <= 0)
        return fail(P4V_ERR_INVALID, "quantize_i8: bad argument");
    Ctx c = Ctx::on(stream, nullptr, 0);
    PackParams p = pack2d(d_x, rows, cols, cols);
    p.Rp = (int)rows; p.Kp = (int)cols_padded; p.dst = d_q; p.C = 1;
    p.scales = d_scales; p.sc_cs = 0; p.blk_mode = 1; p.blk_div = (int)rows_per_scale;
    p.nblk_r = cdiv(rows, rows_per_scale); p.nblk_k = 1; p.lo = lo; p.hi = hi;
    return launch_pack<int8_t>(c, p);
}

int p4v_fake_quant(const float* d_x, int64_t rows, int64_t cols, const float* d_scales, int64_t rows_per_scale,
                   int32_t lo, int32_t hi, float* d_y, void* stream) {
    if (!d_x || !d_scales || !d_y || rows <= 0 || cols <= 0 || rows_per_scale <= 0)
        return fail(P4V_ERR_INVALID, "fake_quant: bad argument");
    const long n = rows * cols;
    hipLaunchKernelGGL(k_fake_quant_rows, dim3((unsigned)std::min<long>(cdiv(n, 256), 65536)), dim3(256), 0,
                       (hipStream_t)stream, d_x, (long)rows, (long)cols, d_scales, (long)rows_per_scale, (float)lo, (float)hi, d_y);
    HIPCHK(hipGetLastError());
    return 0;
}

int p4v_multi_copy(const int64_t* d_table, int32_t n, int64_t index, int64_t max_bytes, void* stream) {
    if (!d_table || n <= 0 || index < 0 || max_bytes <= 0) return fail(P4V_ERR_INVALID, "p4v_multi_copy: bad argument");
    static_assert(sizeof(long) == sizeof(int64_t), "table entries are 64-bit");
    const unsigned gx = (unsigned)std::max<long>(1, std::min<long>(cdiv(max_bytes / 16, 256 * 8), 256));
    hipLaunchKernelGGL(k_multi_copy, dim3(gx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, (const long*)d_table, (long)index);
    HIPCHK(hipGetLastError());
    return 0;
}

// What an event pair measures around NOTHING on an idle stream: the two timestamp packets and the gap between them.  The same
// cost sits inside every timed launch (6-9 us against a rocprofv3 kernel trace of the same launches on MI355X / ROCm 7.2), so
// it is measured when timing is switched on -- minimum over 32 empty pairs on the null stream -- and subtracted from every
// record.  Reported as p4v_kernel_stats.event_overhead_ms; tools/prof_join.py shows the corrected averages next to the trace's.
thread_local double g_evt_overhead_ms = 0.0;
int p4v_stats_enable(int enable) {
    g_stat_on = enable != 0;
    if (g_stat_on) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        double best = 1e9;
        for (int i = 0; i < 32; ++i) {
            HIPCHK(hipEventRecord(a, nullptr));
            HIPCHK(hipEventRecord(b, nullptr));
            HIPCHK(hipEventSynchronize(b));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, a, b));
            best = std::min(best, (double)ms);
        }
        hipEventDestroy(a);
        hipEventDestroy(b);
        g_evt_overhead_ms = best < 1e8 ? best : 0.0;
    }
    return 0;
}

static int stats_drain() {
    for (auto& r : g_stat_recs) {
        HIPCHK(hipEventSynchronize(r.b));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        ms = (float)std::max(0.0, (double)ms - g_evt_overhead_ms);
        if (r.kind == 0 || (r.kind >= 2 && r.kind <= 9) || (r.kind >= 12 && r.kind <= 18)) { g_stats.sweep_i8_ms += ms; g_stats.sweep_i8_launches++; g_stats.sweep_i8_macs += r.macs; g_stats.sweep_i8_alg_macs += r.alg; }
        if (r.kind == 2) { g_stats.sweep6_ms += ms; g_stats.sweep6_launches++; g_stats.sweep6_macs += r.macs; g_stats.sweep6_alg_macs += r.alg; }
        if (r.kind == 3 || r.kind == 4) { g_stats.sweep7_ms += ms; g_stats.sweep7_launches++; g_stats.sweep7_macs += r.macs; g_stats.sweep7_alg_macs += r.alg; }
        if (r.kind == 4) { g_stats.sweep7_twin_ms += ms; g_stats.sweep7_twin_launches++; }
        if (r.kind == 1 || r.kind == 11) { g_stats.sweep_f32_ms += ms; g_stats.sweep_f32_launches++; g_stats.sweep_f32_macs += r.macs; g_stats.sweep_f32_alg_macs += r.alg; }
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
        r.ms = ms;
        g_stat_done.push_back(r);
    }
    g_stat_recs.clear();
    return 0;
}

int p4v_stats_reset(void) {
    int r = stats_drain();
    g_stats = p4v_kernel_stats{};
    g_stat_done.clear();
    g_memo_hits = 0; g_memo_misses = 0;
    return r;
}

int p4v_stats_get(p4v_kernel_stats* out) {
    if (!out) return fail(P4V_ERR_INVALID, "stats_get: null");
    int r = stats_drain();
    g_stats.memo_hits = g_memo_hits; g_stats.memo_misses = g_memo_misses;
    g_stats.event_overhead_ms = g_evt_overhead_ms;
    *out = g_stats;
    return r;
}

int p4v_stats_launches(p4v_launch_record* out, int64_t capacity, int64_t* count) {
    int r = stats_drain();
    if (r) return r;
    if (count) *count = (int64_t)g_stat_done.size();
    if (out)
        for (int64_t i = 0; i < capacity && i < (int64_t)g_stat_done.size(); ++i) {
            const StatRec& s = g_stat_done[(size_t)i];
            out[i] = p4v_launch_record{s.kind, s.stage, s.gx, s.gz, (double)s.ms, 2.0 * s.macs, 2.0 * s.alg, s.bytes};
        }
    return 0;
}

int p4v_prune_counters(int64_t* out4, int reset) {
    if (out4) for (int i = 0; i < 4; ++i) out4[i] = (int64_t)g_prune_cnt[i].load(std::memory_order_relaxed);
    if (reset) for (int i = 0; i < 4; ++i) g_prune_cnt[i].store(0, std::memory_order_relaxed);
    return 0;
}

int p4v_debug_set_variant(int variant, int force_generic) {
    if (variant < 0 || variant >= (1 << 30)) return fail(P4V_ERR_INVALID, "p4v_debug_set_variant: bad variant word");
    if (variant & ~VARIANT_KEPT) return fail(P4V_ERR_INVALID, "p4v_debug_set_variant: bits 0x%x select removed paths", variant & ~VARIANT_KEPT);
    g_variant_word.store(variant | (force_generic ? (1 << 30) : 0), std::memory_order_relaxed);
    return 0;
}

int p4v_debug_set_tuning(int key, int value) {
    if (key < 0 || key >= 16) return fail(P4V_ERR_INVALID, "p4v_debug_set_tuning: unknown key %d", key);
    if (key == TUNE_B1_PATH && tune_b1_removed(value)) return fail(P4V_ERR_INVALID, "p4v_debug_set_tuning: 12 = %d selects a removed path", value);
    g_tune[key].store(value, std::memory_order_relaxed);
    return 0;
}

int p4v_debug_set_arena_gap(size_t bytes) {
    if (bytes % 256) return fail(P4V_ERR_INVALID, "p4v_debug_set_arena_gap: %zu is not a multiple of the arena's 256-byte alignment", bytes);
    g_arena_gap.store(bytes, std::memory_order_relaxed);
    return 0;
}

int p4v_debug_arena_ranges(uint64_t* out, int cap) {
    const int n = (int)g_arena_ranges.size();
    for (int i = 0; out && i < std::min(n, cap); ++i) { out[2 * i] = g_arena_ranges[i].first; out[2 * i + 1] = g_arena_ranges[i].second; }
    return n;
}

static int planes_out(const FusedPlanes& m, uint64_t* out, const char* who, const char* call) {
    if (!out) return fail(P4V_ERR_INVALID, "%s: null pointer", who);
    out[0] = m.off1; out[1] = m.off2; out[2] = (uint64_t)m.rows; out[3] = (uint64_t)m.cols; out[4] = (uint64_t)m.twin;
    return m.rows > 0 ? 0 : fail(P4V_ERR_INVALID, "%s: no %s call on this thread yet", who, call);
}
int p4v_debug_mlp_planes(uint64_t* out) { return planes_out(g_mlp_planes, out, "p4v_debug_mlp_planes", "p4v_mlp_quant_forward"); }
int p4v_debug_attn_planes(uint64_t* out) { return planes_out(g_attn_planes, out, "p4v_debug_attn_planes", "p4v_attn_quant_forward / p4v_wattn_quant_forward"); }
int p4v_debug_qkv_planes(uint64_t* out) {
    const QkvPlanes& m = g_qkv_planes;
    if (!out) return fail(P4V_ERR_INVALID, "p4v_debug_qkv_planes: null pointer");
    const uint64_t v[9] = {m.off_q, m.off_k, m.off_v, (uint64_t)m.Z, (uint64_t)m.rows_q, (uint64_t)m.rows_k, (uint64_t)m.ld_qk, (uint64_t)m.rows_v, (uint64_t)m.ld_v};
    std::copy(v, v + 9, out);
    return m.Z > 0 ? 0 : fail(P4V_ERR_INVALID, "p4v_debug_qkv_planes: no p4v_qkv_attn_quant_forward call on this thread yet");
}

int p4v_debug_sos_sweep(const p4v_matmul_desc* desc, const float* d_A, const float* d_B, const float* d_out, const float* d_grad,
                        int n_cands, int c_lo, int c_hi, int known_cands, float* d_scores, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
    if (!desc || !d_A || !d_B || !d_out || !d_scores || !d_workspace) return fail(P4V_ERR_INVALID, "p4v_debug_sos_sweep: null pointer");
    if (!desc->sos || n_cands < 1 || n_cands > 20 || !sos_split_ok(desc->M, desc->K, desc->N, false))
        return fail(P4V_ERR_INVALID, "p4v_debug_sos_sweep: a split-of-softmax matmul of the one-kernel split search, 1..20 candidates");
    const SosDebugSweep dbg{n_cands, c_lo, c_hi, known_cands, d_scores};
    float* d_split = nullptr;                       // (the sweep selects nothing: split and interval go to scratch)
    CHK(ws_aligned(d_workspace));
    HIPCHK(hipMalloc(&d_split, 2 * sizeof(float)));
    Ctx c = Ctx::on(stream, d_workspace, workspace_bytes);
    g_sos_debug = &dbg;
    const int rc = matmul_impl(desc, {.A = d_A, .B = d_B, .O = d_out, .G = d_grad, .A_iv = d_split + 1, .split = d_split}, Stage{ST_S1}, c);
    g_sos_debug = nullptr;
    (void)hipFree(d_split);
    return rc;
}

int p4v_debug_bound_totals(float* out, int64_t capacity, int64_t* count) {
    if (!out && !count) { g_b1_keep = true; g_b1_totals.clear(); return 0; }
    g_b1_keep = false;
    if (count) *count = (int64_t)g_b1_totals.size();
    if (out) std::copy(g_b1_totals.begin(), g_b1_totals.begin() + std::min<int64_t>(capacity, (int64_t)g_b1_totals.size()), out);
    return 0;
}

int p4v_debug_prune_tables(int32_t* out, int64_t capacity, int64_t* count) {
    if (!out && !count) { g_tables_keep = true; g_tables.clear(); return 0; }
    g_tables_keep = false;
    if (count) *count = (int64_t)g_tables.size();
    if (out) std::copy(g_tables.begin(), g_tables.begin() + std::min<int64_t>(capacity, (int64_t)g_tables.size()), out);
    return 0;
}

// The decision chain of run_pass_pruned_impl -- same launchers, same order, same branches -- with the three sweeps replaced by the
// tables k_finish would leave, built on the host from the caller's totals T and the ranges the kernels wrote (the reads this
// emulation needs are its own: `host_reads` is the pass's "the host reads the survivors", the early exit through select_from_b1).
int p4v_debug_prune_decide(const float* d_SA, const float* d_SA2, const float* d_T, const float* d_cands, int C, int nj, int virt,
                           int honour_blk, int host_reads, int32_t* d_ranges, int32_t* d_rblk, int32_t* d_best, float* d_interval,
                           int32_t* d_best_out, int32_t* info, void* stream) {
    if (!d_SA || !d_T || !d_cands || !d_ranges || !d_rblk || !d_best || !d_interval || !d_best_out || !info)
        return fail(P4V_ERR_INVALID, "p4v_debug_prune_decide: null pointer");
    if (C < 1 || nj < 1 || nj > 4096 || (virt && nj == 1))
        return fail(P4V_ERR_INVALID, "p4v_debug_prune_decide: 1 <= C, 1 <= nj <= 4096, the synthetic candidate needs nj > 1");
    Ctx c = Ctx::on(stream, nullptr, 0);
    const size_t tab = (size_t)C * nj;
    const float ninf = -INFINITY;
    struct Scratch { float* p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } } dev;
    HIPCHK(hipMalloc(&dev.p, sizeof(float) * (3 * tab + nj)));
    PrunePlan pl{};
    pl.virt = virt != 0;
    pl.hull_selects = prune_hull_selects(false, true, pl.virt, nj);
    PruneBufs b{};
    b.tab = tab;
    b.SA = const_cast<float*>(d_SA); b.SB = dev.p; b.S2 = b.SB + tab; b.SA2 = b.S2 + tab; b.vrow = b.SA2 + tab;
    b.r1 = d_ranges; b.r2 = b.r1 + 2; b.r3 = b.r1 + 4;
    b.best_idx = d_best; b.rblk2 = d_rblk; b.rblk3 = d_rblk + 2 * nj;
    Pass ps{};
    ps.eq_n = C; ps.nj = nj; ps.cands = d_cands; ps.cand_cs = nj; ps.cand_js = 1; ps.cand_off = 0;
    ps.interval = d_interval; ps.out_js = 1; ps.out_off = 0; ps.aux_div = 1.0f; ps.best_out = d_best_out;
    std::vector<float> T(tab), SA2(d_SA2 ? tab : 0), h(tab);
    std::vector<int> best(nj), rblk(2 * (size_t)nj);
    int r[2] = {0, 0};
    CHK(q_fill(c, d_ranges, 0xff, sizeof(int) * 6));                 // what a branch does not write stays -1
    CHK(q_fill(c, d_rblk, 0xff, sizeof(int) * 4 * nj));
    CHK(q_fill(c, d_best, 0xff, sizeof(int) * nj));
    CHK(q_d2h(c, T.data(), d_T, sizeof(float) * tab));
    if (d_SA2) CHK(q_d2h(c, SA2.data(), d_SA2, sizeof(float) * tab));
    info[0] = pl.hull_selects; info[1] = 0; info[2] = 0;            // hull_selects, tier 2 ran, exit (0 merge, 1 / 2 no stage B2 after tier 1 / 2)
    // the table a sweep of T over the device-side range `rng` (+ the per-block ranges `blk`) leaves in `dst`
    auto sweep = [&](const std::vector<float>& src, float* dst, const int* rng, const int* blk) -> int {
        CHK(q_d2h(c, r, rng, sizeof r));
        if (blk) CHK(q_d2h(c, rblk.data(), blk, sizeof(int) * 2 * nj));
        CHK(q_sync(c));
        std::fill(h.begin(), h.end(), ninf);
        for (int cc = std::max(r[0], 0); cc < std::min(r[1], C); ++cc)
            for (int j = 0; j < nj; ++j)
                if (!blk || (cc >= rblk[2 * j] && cc < rblk[2 * j + 1])) h[(size_t)cc * nj + j] = src[(size_t)cc * nj + j];
        CHK(q_h2d(c, dst, h.data(), sizeof(float) * tab));
        return q_sync(c);
    };
    PruneParams pp{b.SA, b.SB, C, nj, prune_margin(), b.r1, b.r1, pl.virt ? 1 : 0, b.best_idx, ps.cands, ps.cand_cs, ps.cand_js, ps.cand_off, b.vrow};
    CHK(launch_pick(c, pp));
    if (pl.virt) {              // stage B1 on the synthetic candidate: row 0 holds every block's winner's total
        CHK(q_d2h(c, best.data(), b.best_idx, sizeof(int) * nj));
        CHK(q_sync(c));
        std::fill(h.begin(), h.end(), ninf);
        for (int j = 0; j < nj; ++j) {
            if (best[j] < 0 || best[j] >= C) return fail(P4V_ERR_INVALID, "p4v_debug_prune_decide: k_prune_pick left winner %d in block %d", best[j], j);
            h[j] = T[(size_t)best[j] * nj + j];
        }
        CHK(q_h2d(c, b.SB, h.data(), sizeof(float) * tab));
        CHK(q_sync(c));
    } else CHK(sweep(T, b.SB, b.r1, nullptr));
    int* hm = host_reads ? host_mirror(c) : nullptr;
    SelectParams hsl{b.SB, ps.eq_n, ps.nj, ps.cands, ps.cand_cs, ps.cand_js, ps.cand_off, pl.hull_selects ? ps.interval : nullptr,
                     ps.out_js, ps.out_off, ps.aux_out, ps.aux_div, nullptr, 0, ps.best_out};
    attach_mirror(hsl);
    pp.r_out = b.r2; pp.rblk = b.rblk2;
    CHK(launch_hull(c, pp, hsl, hm, MIR_R1, MIR_RB1));
    Survivors s1, s2;
    if (host_reads) {
        CHK(read_survivors(c, b.r2, hm, MIR_R1, MIR_RB1, nj, s1));
        if (!s1.count) { info[2] = 1; CHK(select_from_b1(c, ps, pl, b)); return q_sync(c); }
    }
    bool second_tier = false;
    if (d_SA2) {                // stage A2: the caller's partial sums where the first hull's ranges let a sweep evaluate them
        CHK(sweep(SA2, b.SA2, b.r2, honour_blk ? b.rblk2 : nullptr));
        pp.SA = b.SA2; pp.r_out = b.r3; pp.rblk = b.rblk3;
        CHK(launch_hull(c, pp, hsl, hm, MIR_R2, MIR_RB2));
        second_tier = true; info[1] = 1;
        if (host_reads) {
            CHK(read_survivors(c, b.r3, hm, MIR_R2, MIR_RB2, nj, s2));
            if (!s2.count) { info[2] = 2; CHK(select_from_b1(c, ps, pl, b)); return q_sync(c); }
        }
    }
    CHK(sweep(T, b.S2, second_tier ? b.r3 : b.r2, !honour_blk ? nullptr : second_tier ? b.rblk3 : b.rblk2));      // stage B2
    if (pl.virt) CHK(enqueue(c, KERN(MergeVirtParams, k_merge_virtual), dim3(cdiv(ps.nj, 64)), dim3(64), 0, MergeVirtParams{b.S2, b.SB, b.best_idx, ps.nj}));
    else CHK(enqueue(c, KERN(MergeParams, k_merge_scores), dim3(cdiv((long)b.tab, 256)), dim3(256), 0, MergeParams{b.S2, b.SB, (int)b.tab}));
    CHK(launch_pass_select(c, ps, b.S2));
    return q_sync(c);
}

int p4v_debug_topk_rows(const float* d_mass, int segs, int n, int k, int32_t* d_idx, void* stream) {
    if (!d_mass || !d_idx || segs <= 0 || n <= 0 || k <= 0 || k > n) return fail(P4V_ERR_INVALID, "p4v_debug_topk_rows: bad argument");
    hipLaunchKernelGGL(k_topk_rows, dim3(segs), dim3(1024), 0, (hipStream_t)stream, TopkParams{d_mass, n, k, d_idx});
    HIPCHK(hipGetLastError());
    return 0;
}

int p4v_debug_pack_dual(const float* d_x, long rows, long cols, long cols_padded, int sos, int lo, int hi, int qmax,
                        const float* d_scale, float const_scale, int8_t* d_q1, int8_t* d_q2, void* stream) {
    if (!d_x || !d_scale || !d_q1 || !d_q2 || rows <= 0 || cols <= 0 || cols_padded % 64 || cols_padded < cols ||
        lo > 0 || hi < 0 || lo < -128 || hi > 127 || qmax < 2 || qmax > 128 || (!sos && !(const_scale > 0.0f)))
        return fail(P4V_ERR_INVALID, "p4v_debug_pack_dual: bad argument");
    PackParams p1 = pack2d(d_x, rows, cols, cols);
    p1.Rp = (int)rows; p1.Kp = (int)cols_padded; p1.C = 1; p1.scales = d_scale; p1.qm1 = (float)(qmax - 1);
    PackParams p2 = p1;
    p1.dst = d_q1; p2.dst = d_q2;
    if (sos) {
        p1.mode = PACK_SOS_HI; p2.mode = PACK_SOS_LO;
    } else {              // the post-GELU pair: [0, hi] on *d_scale, [lo, 0] on const_scale
        p1.lo = 0; p1.hi = hi; p2.lo = lo; p2.hi = 0; p2.scales = nullptr; p2.neg_scale = const_scale;
    }
    if (!dual_pack_ok(p1, p2)) return fail(P4V_ERR_INVALID, "p4v_debug_pack_dual: not a dual pair");
    Ctx c = Ctx::on(stream, nullptr, 0);
    const long total = rows * (cols_padded / 16);
    if (total >= (1L << 31)) return fail(P4V_ERR_UNSUPPORTED, "p4v_debug_pack_dual: plane too large");
    return enqueue(c, KERN(PackDualParams, k_pack_dual), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 64)), dim3(256), 0,
                   PackDualParams{p1, p2});
}

int p4v_debug_pack_cands(const float* d_x, long rows, long cols, long rows_padded, long cols_padded, int layout, int lo, int hi,
                         const float* d_scales, int n_cands, const int* d_crange, const unsigned char* d_done, int live_max,
                         int general, int8_t* d_q, void* stream) {
    if (!d_x || !d_scales || !d_q || rows <= 0 || cols <= 0 || rows_padded < rows || cols_padded % 64 || cols_padded < cols ||
        layout < 0 || layout > 3 || (layout == 3 && rows_padded % 64) || lo > hi || lo < -128 || hi > 127 || n_cands <= 0 ||
        (d_done && !d_crange) || (live_max >= 0 && !d_crange))
        return fail(P4V_ERR_INVALID, "p4v_debug_pack_cands: bad argument");
    Ctx c = Ctx::on(stream, nullptr, 0);
    cvt_bias(c);
    PackParams p = pack2d(d_x, rows, cols, cols);
    p.Rp = (int)rows_padded; p.Kp = (int)cols_padded; p.dst = d_q; p.C = n_cands; p.c_inner = layout;
    p.scales = d_scales; p.sc_cs = 1; p.lo = lo; p.hi = hi;
    p.crange = d_crange; p.c_base = 0; p.done = d_done;
    g_pack_general.store(general ? 1 : 0, std::memory_order_relaxed);
    const int r = launch_pack<int8_t>(c, p, live_max);
    g_pack_general.store(0, std::memory_order_relaxed);
    return r;
}

int p4v_debug_gather_im2col(int batch, int in_channels, int height, int width, int kernel_h, int kernel_w, int stride_h, int stride_w,
                            int pad_h, int pad_w, int dil_h, int dil_w, const float* d_x, const int32_t* d_idx, int k, float* d_dst,
                            void* stream) {
    if (!d_x || !d_idx || !d_dst || k <= 0 || batch <= 0 || in_channels <= 0 || height <= 0 || width <= 0 || kernel_h <= 0 ||
        kernel_w <= 0 || stride_h <= 0 || stride_w <= 0 || pad_h < 0 || pad_w < 0 || dil_h <= 0 || dil_w <= 0)
        return fail(P4V_ERR_INVALID, "p4v_debug_gather_im2col: bad argument");
    const int num_h = height + 2 * pad_h - dil_h * (kernel_h - 1) - 1, num_w = width + 2 * pad_w - dil_w * (kernel_w - 1) - 1;
    if (num_h < 0 || num_w < 0) return fail(P4V_ERR_INVALID, "p4v_debug_gather_im2col: bad geometry");
    const int fh = num_h / stride_h + 1, fw = num_w / stride_w + 1;
    PackParams p{};         // the conv view exactly as ConvCall::x_operand builds it for the flat layout (Z = 1, rows = b * L)
    p.src = d_x; p.conv = 1; p.ic = in_channels; p.H = height; p.W = width; p.kh = kernel_h; p.kw = kernel_w;
    p.sh = stride_h; p.sw = stride_w; p.ph = pad_h; p.pw = pad_w; p.dh = dil_h; p.dw = dil_w;
    p.fw = fw; p.L = fh * fw;
    p.Z = 1; p.s_z = 0; p.R = batch * fh * fw; p.K = in_channels * kernel_h * kernel_w; p.nblk_r = 1; p.nblk_k = 1;
    p.mode = PACK_RAW;
    Ctx c = Ctx::on(stream, nullptr, 0);
    const long total = (long)k * p.K;
    return enqueue(c, KERN(GatherIm2colParams, k_gather_im2col), dim3((unsigned)std::min<long>(cdiv(total, 256), 256L * 16)), dim3(256), 0,
                   GatherIm2colParams{p, d_idx, k, d_dst});
}

int p4v_debug_prep_epi6(const float* d_o, const float* d_wt, const float* d_bias, long o_ss, long o_ts, int sr, int tr,
                        int bias_on_t, int wt_mode, int transposed, float* d_e, void* stream) {
    if (!d_o || !d_bias || !d_e || (wt_mode == 1 && !d_wt) || sr <= 0 || tr <= 0 || wt_mode < 0 || wt_mode > 4)
        return fail(P4V_ERR_INVALID, "p4v_debug_prep_epi6: bad argument");
    PrepEpi6Params pe{};
    pe.O = d_o; pe.Wt = d_wt ? d_wt : d_o; pe.bias = d_bias; pe.o_ss = o_ss; pe.o_ts = o_ts; pe.SR = sr; pe.TR = tr;
    pe.bias_on_t = bias_on_t ? 1 : 0; pe.wt_mode = wt_mode; pe.transposed = transposed ? 1 : 0;
    pe.stiles = cdiv(sr, 256); pe.ttiles = cdiv(tr, 64); pe.E = d_e;
    Ctx c = Ctx::on(stream, nullptr, 0);
    return enqueue(c, KERN(PrepEpi6Params, k_prep_epi6), dim3((unsigned)std::min<long>((long)pe.stiles * pe.ttiles, 256L * 32)), dim3(256), 0, pe);
}

int p4v_pack_plane_i8(const p4v_plane_desc* d, const float* d_x, const float* d_scales, int8_t* d_q, void* stream) {
    if (!d || !d_x || !d_q || d->rows <= 0 || d->cols <= 0 || d->cols_padded % 64 || d->cols_padded < d->cols)
        return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: bad argument");
    if (d->mode != P4V_PLANE_SYM && d->mode != P4V_PLANE_SOS_HI && d->mode != P4V_PLANE_SOS_LO && d->mode != P4V_PLANE_TWIN)
        return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: unknown mode %d", d->mode);
    if (d->mode == P4V_PLANE_TWIN && (d->lo > 0 || d->hi < 0 || !(d->const_scale > 0.0f)))
        return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: the merged twin plane needs lo <= 0 <= hi and const_scale > 0");
    if (d->mode != P4V_PLANE_SYM && !d_scales) return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: split-of-softmax planes need d_scales = &split");
    if (d->mode == P4V_PLANE_SYM && d_scales && d->rows_per_scale <= 0) return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: rows_per_scale");
    if (d->lo < -128 || d->hi > 127 || d->qmax < 2 || d->qmax > 128) return fail(P4V_ERR_INVALID, "p4v_pack_plane_i8: grid wider than int8");
    Ctx c = Ctx::on(stream, nullptr, 0);
    cvt_bias(c);     // (first use of the process: the conversion quant16_sat8 relies on is probed, into a scratch of the library's own)
    PackParams p = pack2d(d_x, d->rows, d->cols, d->cols);
    p.Rp = (int)d->rows; p.Kp = (int)d->cols_padded; p.dst = d_q; p.C = 1;
    p.scales = d_scales; p.sc_cs = 0; p.neg_scale = d->const_scale;
    p.lo = d->lo; p.hi = d->hi; p.qm1 = (float)(d->qmax - 1);
    if (d->mode == P4V_PLANE_SYM) {
        p.mode = PACK_SYM;
        if (d_scales) { p.blk_mode = 1; p.blk_div = (int)d->rows_per_scale; p.nblk_r = cdiv(d->rows, d->rows_per_scale); p.nblk_k = 1; }
    } else if (d->mode == P4V_PLANE_TWIN) {
        p.mode = PACK_TWIN_I8;
    } else {
        p.mode = d->mode == P4V_PLANE_SOS_HI ? PACK_SOS_HI : PACK_SOS_LO;
    }
    return launch_pack<int8_t>(c, p);
}

int p4v_export_quantize(const p4v_export_desc* d, const float* d_src, const float* d_scale1, const float* d_scale2,
                        void* d_dst, void* stream) {
    if (!d || !d_src || !d_scale1 || !d_dst) return fail(P4V_ERR_INVALID, "p4v_export_quantize: null pointer");
    if (d->mode < P4V_EXPORT_SYM_I8 || d->mode > P4V_EXPORT_SOS_U8) return fail(P4V_ERR_INVALID, "p4v_export_quantize: unknown mode %d", d->mode);
    if (d->mode == P4V_EXPORT_SOS_U8 && !d_scale2) return fail(P4V_ERR_INVALID, "p4v_export_quantize: the split-of-softmax format needs d_scale2 = A_interval");
    ExportParams p{};
    long total = 1;
    for (int i = 0; i < 4; ++i) {
        if (d->dims[i] <= 0 || d->scale1_div[i] <= 0 || (d_scale2 && d->scale2_div[i] <= 0))
            return fail(P4V_ERR_INVALID, "p4v_export_quantize: non-positive dimension / block size");
        p.d[i] = d->dims[i]; p.ss[i] = d->src_stride[i];
        p.s1s[i] = d->scale1_stride[i]; p.s1d[i] = d->scale1_div[i];
        p.s2s[i] = d->scale2_stride[i]; p.s2d[i] = d_scale2 ? d->scale2_div[i] : 1;
        total *= d->dims[i];
    }
    p.src = d_src; p.s1 = d_scale1; p.s2 = d_scale2; p.s2_const = d->scale2_const;
    p.mode = d->mode == P4V_EXPORT_SYM_I8 ? EXP_SYM_I8 : d->mode == P4V_EXPORT_SYM_F32 ? EXP_SYM_F32
           : d->mode == P4V_EXPORT_GELU_U8 ? EXP_GELU_U8 : EXP_SOS_U8;
    p.lo1 = d->lo1; p.hi1 = d->hi1; p.lo2 = d->lo2; p.hi2 = d->hi2; p.qm1 = (float)(d->qmax - 1);
    p.dst = d_dst;
    const unsigned blocks = (unsigned)std::min<long>(cdiv(total, 256), 256L * 32);
    hipLaunchKernelGGL(k_export, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
