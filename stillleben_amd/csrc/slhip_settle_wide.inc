// slhip_settle_wide.inc -- the LOCKSTEP settle pipeline (included by slhip_settle.hip inside its
// anonymous namespace; shares every device function with the persistent kernel, so the arithmetic
// -- and with it the bit-exact contract with oracle/settle_ref.c -- is the same code).
//
// k_settle keeps one scene per wave for all 400 steps: with 256 VGPRs and ~20 KiB of LDS per scene
// at most 8 scenes live on a CU, every phase of a step runs on as many lanes as ONE scene offers
// (SQ counters: 8.4 of 64 lanes active) and a launch ends with its slowest scene.  Here every step is
// six launches over the WHOLE batch, with the scenes' state in HBM/L2 between them:
//
//   k_w_begin      wave = scene        integrate forces, table contacts, broadphase -> hull pairs, appended to the step's work list
//   k_w_gjk_first  lane = hull pair of any scene   ONE GJK iteration (pair cache warm start); unfinished pairs -> second list
//   k_w_gjk_rest   lane = unfinished pair          the whole run from the start; both refresh the manifold the pair had
//   k_w_manifold   16 lanes = contact pair of any scene that is new or lost a point: its face manifold (clipped support features)
//   k_w_finish     wave = scene        contact list, groups, wake, prep, colouring, the scene's solver cost class
//   k_w_solve      wave = one, two or four scenes by the LDS a scene's solve needs this step (SLHIP_SOLVE_SPW caps it; costliest first,
//                                      neighbours in the cost order side by side) 4 + 4 Gauss-Seidel sweeps,
//                                      integrate, sleep, (frame end) redrop
//
// The narrowphase kernels fill their waves with pairs (no per-scene LDS at all), the per-scene
// kernels need a few KiB of LDS and far fewer registers than the fused kernel, so several thousand
// scenes are in flight at once and a step costs the latency of its slowest phase, not of its slowest
// scene.  All per-pair / per-contact orders are the persistent kernel's (and the oracle's).

struct WideHdr {
    int n_hp, n_groups, n_plane_groups, n_active, n_active_before_pairs, ncol, status, n_hulls;
    int hp_overflow, hp_found;           // the step's broadphase found hp_found hull pairs; beyond the list's capacity they were dropped (counted)
    int g_overflow;                      // the step's broadphase found more touching body pairs than the scene's group list holds (dropped, counted)
    int lds_need, lds_class;             // k_w_finish: bytes of LDS the scene's solve wants this step, its wave class (below)
};
// persistent table contacts of one body (oracle pplane): the vertex numbers of the last step's contacts and where their
// impulses lie in the step's impulse array
struct PlanePM { int stamp, count, c_off, id[4], pad; };
static_assert(sizeof(PlanePM) == 32, "PlanePM layout");

// Pair cache entry (16 bytes; oracle: scene_ws.cache + the way to scene_ws.pm): x = simplex size (2 bits) | the pair produced
// contacts (1) | the step that wrote the entry (29); y = simplex vertices 0 and 1, z = vertex 2 | the pair's slot in that step's
// pair list << 16 -- the way from a hull pair to the manifold the previous step left it; w = 1 + (hull a | hull b << 16), the
// key of the hashed form (0: free slot).  A simplex vertex is (vertex of A | vertex of B << 8): hulls have at most 64 vertices.
__device__ __forceinline__ int cache_x(int seed_n, bool has, unsigned step) { return (seed_n & 3) | ((has ? 1 : 0) << 2) | (int)(step << 3); }
__device__ __forceinline__ int sv_pack(int idx) { return (idx & 0xff) | ((idx >> 16) << 8); }
__device__ __forceinline__ int sv_unpack(int c) { return (c & 0xff) | (((c >> 8) & 0xff) << 16); }

// per (scene): what the capacities cost since the cold start (slhip_settle_caps)
enum { kCapSpillSteps = 0, kCapContactDropSteps, kCapPairDropSteps, kCapMaxContacts, kCapMaxPairs, kCapReducedSteps, kCapGroupDropSteps, kCapContactSum, kCapWords = 8 };
constexpr unsigned short kCulled = 0xffff;   // k_w_finish, hp_off: the pair offers its point but pair_contact_budget keeps it out of the solver

__device__ const float kNoImpulse[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // the impulses of a manifold that was out of the solver (pair_contact_budget)

struct WideBufs {
    WideHdr* hdr;            // [S]
    WBody* wb;               // [S][nb_cap]
    HullRef* lh;             // [S][lh_cap]
    int* body_lh;            // [S][nb_cap + 1]
    HullPair* hp;            // [S][p_cap] the step's candidate hull pairs
    unsigned short* hp_off;  // [S][p_cap + 1] k_w_finish: contacts the pair keeps, then the pair's first contact
    unsigned short* hp_grp;  // [S][p_cap]     k_w_finish: the pair's group
    MainResult* mr;          // [S][p_cap]
    StagePt* stage;          // [S][p_cap][4] the points of a contact pair's manifold between the stages of the narrowphase
    Contact* ac;             // [S][c_cap]
    Group* groups;           // [S][g_cap]
    unsigned short* order;   // [S][o_stride]: groups colour by colour [g_cap], then the colours' first slots
    unsigned* lpt_count;     // [3 wave classes][32 cost classes x 8 shards] scenes per wave class (k_w_finish: by the LDS the scene's solve
                             // needs this step -- 0: a wave of its own, 1: two scenes per wave, 2: four), class of solver cost (the
                             // sequential chain of a sweep / 8) and shard (scene & 7); then [3][8] the wave classes' totals by shard; zeroed by k_w_begin
    unsigned short* lpt_table; // [3][256][ceil(S / 8)] their scenes in arrival order: k_w_solve's blocks take the costliest class first
    unsigned* work;          // [5][S * p_cap]: hull pairs of ALL scenes side by side (scene << pair_bits | pair).  Regions 0-2 = list 0,
                             // every candidate pair of the step by size class (the larger hull has <= 16 / <= 32 / more vertices: a support
                             // scan costs a lane as many 8-vertex batches as its hull has, and a wave as many as its largest hull);
                             // region 3 = list 1, the pairs whose GJK run is not over after its first iteration; region 4 = list 2, the
                             // contact pairs whose manifold is built in this step (k_w_manifold).  Lists 1 and 2 are appended block by block while list 0 is walked in
                             // order, so they inherit its grouping
    PM* pm;                  // [2][S][p_cap] persistent manifolds by step parity and pair slot (k_w_finish reads the previous
                             // step's while it writes this step's)
    float* lnout;            // [S][c_cap] the normal impulses the last step's contacts ended with (k_w_solve)
    PlanePM* pp;             // [S][nb_cap]
    unsigned* caps;          // [S][kCapWords] (slhip_settle_caps)
    unsigned* work_count;    // lengths: [2] list 1, [3] list 2 (bumped together as one 64-bit atomic), [8..10] list 0 by class; zeroed by the
                             // prologue and, for the next step, by k_w_finish
    int nb_cap, lh_cap;
    int p_cap, c_cap;        // capacities of a scene's hull-pair and contact lists (slhip_settle_params)
    int g_cap, o_stride;     // groups per scene: nb_cap table groups + min(p_cap, body pairs); stride of `order`
    int pair_bits;           // work list entries: scene << pair_bits | pair
    int solve_lds;           // bytes of LDS of a solver wave (host: slhip_settle); the wave classes are its quarters
    int solve_max_class;     // 2: waves of up to four scenes; 1: up to two; 0: one scene per wave (SLHIP_SOLVE_SPW)
};
constexpr int kLptWords = 3 * 256 + 3 * 8;      // ... the totals in eight shards each (scene & 7): 16384 atomics on one address queue up

__host__ __device__ inline size_t wide_align(size_t x) { return (x + 255u) & ~(size_t)255u; }

// groups of a scene: one per body against the table + one per body pair with candidate hull pairs -- at most every body pair, at
// most the hull-pair capacity, and as many as the caller sized (slhip_settle_params.max_body_pairs_per_scene; 0: twelve neighbours
// per body on average, so that the kernels' LDS copies stay bounded for scenes of hundreds of bodies); a body pair beyond that is
// dropped like a hull pair beyond the list's capacity, and counted in a word of its own
__host__ __device__ inline int wide_g_cap(int nb_cap, int p_cap, int bp_cap)
{
    long long pairs = (long long)nb_cap * (nb_cap - 1) / 2;
    if (pairs > p_cap) pairs = p_cap;
    const long long lim = bp_cap > 0 ? (long long)bp_cap : 12ll * nb_cap + 64;
    if (pairs > lim) pairs = lim;
    return nb_cap + (int)pairs;
}

inline uint64_t wide_bytes(uint32_t n, int nb_cap, int lh_cap, int p_cap, int c_cap, int bp_cap)
{
    const size_t g_cap = (size_t)wide_g_cap(nb_cap, p_cap, bp_cap), o_stride = 2 * g_cap + 66;
    uint64_t b = 0;
    b += wide_align((size_t)n * sizeof(WideHdr));
    b += wide_align((size_t)n * nb_cap * sizeof(WBody));
    b += wide_align((size_t)n * lh_cap * sizeof(HullRef));
    b += wide_align((size_t)n * (nb_cap + 1) * sizeof(int));
    b += wide_align((size_t)n * p_cap * sizeof(HullPair));
    b += wide_align((size_t)n * (p_cap + 1) * sizeof(unsigned short));
    b += wide_align((size_t)n * p_cap * sizeof(unsigned short));
    b += wide_align((size_t)n * p_cap * sizeof(MainResult));
    b += wide_align((size_t)n * p_cap * 4 * sizeof(StagePt));
    b += wide_align((size_t)n * c_cap * sizeof(Contact));
    b += wide_align((size_t)n * g_cap * sizeof(Group));
    b += wide_align((size_t)n * o_stride * sizeof(unsigned short));
    b += wide_align((size_t)5 * n * p_cap * sizeof(unsigned));
    b += wide_align((size_t)2 * n * p_cap * sizeof(PM));
    b += wide_align((size_t)n * c_cap * sizeof(float));
    b += wide_align((size_t)n * nb_cap * sizeof(PlanePM));
    b += wide_align((size_t)n * kCapWords * sizeof(unsigned));
    b += wide_align(64);
    b += wide_align(kLptWords * sizeof(unsigned));
    b += wide_align((size_t)3 * 256 * ((n + 7u) / 8u) * sizeof(unsigned short));
    return b;
}

inline WideBufs wide_carve(char* base, uint32_t n, int nb_cap, int lh_cap, int p_cap, int c_cap, int bp_cap)
{
    WideBufs B;
    B.nb_cap = nb_cap; B.lh_cap = lh_cap; B.p_cap = p_cap; B.c_cap = c_cap;
    B.g_cap = wide_g_cap(nb_cap, p_cap, bp_cap); B.o_stride = 2 * B.g_cap + 66;
    B.pair_bits = 1;
    while ((1 << B.pair_bits) < p_cap) ++B.pair_bits;
    char* p = base;
    auto take = [&](size_t bytes) { char* r = p; p += wide_align(bytes); return r; };
    B.hdr = reinterpret_cast<WideHdr*>(take((size_t)n * sizeof(WideHdr)));
    B.wb = reinterpret_cast<WBody*>(take((size_t)n * nb_cap * sizeof(WBody)));
    B.lh = reinterpret_cast<HullRef*>(take((size_t)n * lh_cap * sizeof(HullRef)));
    B.body_lh = reinterpret_cast<int*>(take((size_t)n * (nb_cap + 1) * sizeof(int)));
    B.hp = reinterpret_cast<HullPair*>(take((size_t)n * p_cap * sizeof(HullPair)));
    B.hp_off = reinterpret_cast<unsigned short*>(take((size_t)n * (p_cap + 1) * sizeof(unsigned short)));
    B.hp_grp = reinterpret_cast<unsigned short*>(take((size_t)n * p_cap * sizeof(unsigned short)));
    B.mr = reinterpret_cast<MainResult*>(take((size_t)n * p_cap * sizeof(MainResult)));
    B.stage = reinterpret_cast<StagePt*>(take((size_t)n * p_cap * 4 * sizeof(StagePt)));
    B.ac = reinterpret_cast<Contact*>(take((size_t)n * c_cap * sizeof(Contact)));
    B.groups = reinterpret_cast<Group*>(take((size_t)n * B.g_cap * sizeof(Group)));
    B.order = reinterpret_cast<unsigned short*>(take((size_t)n * B.o_stride * sizeof(unsigned short)));
    B.work = reinterpret_cast<unsigned*>(take((size_t)5 * n * p_cap * sizeof(unsigned)));
    B.pm = reinterpret_cast<PM*>(take((size_t)2 * n * p_cap * sizeof(PM)));
    B.lnout = reinterpret_cast<float*>(take((size_t)n * c_cap * sizeof(float)));
    B.pp = reinterpret_cast<PlanePM*>(take((size_t)n * nb_cap * sizeof(PlanePM)));
    B.caps = reinterpret_cast<unsigned*>(take((size_t)n * kCapWords * sizeof(unsigned)));
    B.work_count = reinterpret_cast<unsigned*>(take(64));
    B.lpt_count = reinterpret_cast<unsigned*>(take(kLptWords * sizeof(unsigned)));
    B.lpt_table = reinterpret_cast<unsigned short*>(take((size_t)3 * 256 * ((n + 7u) / 8u) * sizeof(unsigned short)));
    B.solve_lds = 0; B.solve_max_class = 2;
    return B;
}

// The pair cache of one scene.  An entry lives as long as its pair stays a broadphase candidate: it is used by the step after the one
// that wrote it and by no later one (oracle hull_pair_contacts; PhysX drops a pair's cache with the pair [ext]).  Up to
// SLHIP_PAIR_CACHE_DENSE_HULLS hulls: ONE dense [hulls]^2 table, stale entries told by their step stamp.  Beyond: TWO open-addressing
// hash tables (linear probing, key word claimed by compare-and-swap), by step parity -- a step looks its pairs up in the table the
// previous step filled and files them in its own, which k_w_finish of the step before has emptied: no deletions, never more than
// one step's pairs in a table.  `stride` = entries per scene (hashed: two tables of stride / 2, a power of two).
struct PairCache {
    int4* base;
    unsigned stride;
    int hashed;
};
// `claim`: the slot the pair's entry of THIS step goes to (hashed: found or claimed in the table of `parity`); otherwise the slot
// the previous step may have left (hashed: looked up in the table of `parity`, nullptr when the pair is not in it)
__device__ __forceinline__ int4* pair_cache_slot(const PairCache& pc, int s, int n_hulls, int la, int lb, unsigned parity, bool claim)
{
    int4* tab = pc.base + (size_t)s * pc.stride;
    if (!pc.hashed) {
        if (n_hulls <= 0 || (unsigned)n_hulls * (unsigned)n_hulls > pc.stride) return nullptr;
        return tab + (size_t)la * n_hulls + lb;
    }
    const unsigned half = pc.stride >> 1, mask = half - 1u;
    tab += (size_t)(parity & 1u) * half;
    const unsigned key = ((unsigned)la | ((unsigned)lb << 16)) + 1u;
    unsigned h = (key * 2654435761u) >> 7;
    for (unsigned probe = 0; probe < half; ++probe, ++h) {
        int4* e = tab + (h & mask);
        unsigned k = (unsigned)e->w;
        if (k == 0u) {
            if (!claim) return nullptr;
            // (a key, once written, stays until the table is emptied: a stale zero from the L1 is corrected by the swap's return value)
            k = atomicCAS(reinterpret_cast<unsigned*>(&e->w), 0u, key);
            if (k == 0u) k = key;
        }
        if (k == key) return e;
    }
    return nullptr;                            // (a table holds four slots per list entry: never full)
}

// dword copies between LDS and global memory by the lanes of one wave
// (8-byte units, four loads in flight per lane: a dword-by-dword loop pays one memory round trip per iteration, and the waves of
// these kernels have nothing else to hide it behind.  Both pointers 8-byte aligned; a trailing dword is copied by itself.)
__device__ __forceinline__ void lanes_copy(void* dst, const void* src, int bytes, int hl, int n_lanes)
{
    uint2* d = reinterpret_cast<uint2*>(dst);
    const uint2* q = reinterpret_cast<const uint2*>(src);
    const int n8 = bytes >> 3;
    for (int k = hl; k < n8; k += 4 * n_lanes) {
        const int k1 = k + n_lanes, k2 = k + 2 * n_lanes, k3 = k + 3 * n_lanes;
        uint2 a0 = q[k], a1 = a0, a2 = a0, a3 = a0;
        if (k1 < n8) a1 = q[k1];
        if (k2 < n8) a2 = q[k2];
        if (k3 < n8) a3 = q[k3];
        d[k] = a0;
        if (k1 < n8) d[k1] = a1;
        if (k2 < n8) d[k2] = a2;
        if (k3 < n8) d[k3] = a3;
    }
    if ((bytes & 4) && hl == 0) reinterpret_cast<unsigned*>(dst)[2 * n8] = reinterpret_cast<const unsigned*>(src)[2 * n8];
}
__device__ __forceinline__ void wave_copy_words(void* dst, const void* src, int bytes, int lane) { lanes_copy(dst, src, bytes, lane, 64); }

// ---- once per cold settle call: local hull table of every scene, pair cache cleared -----------------------
__global__ __launch_bounds__(64) void k_w_prologue(const slhip_settle_scene* __restrict__ scenes,
                                                  const slhip_body* __restrict__ bodies_all,
                                                  const slhip_hull* __restrict__ hulls, WideBufs W,
                                                  ProfScratch* prof_all, PairCache pc)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const slhip_settle_scene sc = scenes[s];
    const slhip_body* bodies = bodies_all + sc.body_begin;
    const int nb = (int)(sc.body_end - sc.body_begin);
    WideHdr* H = W.hdr + s;
    HullRef* lh = W.lh + (size_t)s * W.lh_cap;
    int* body_lh = W.body_lh + (size_t)s * (W.nb_cap + 1);
    if (s == 0 && lane < 16) W.work_count[lane] = 0u;
    if (s == 0) for (int k = lane; k < kLptWords; k += 64) W.lpt_count[k] = 0u;
    if (lane < kCapWords) W.caps[kCapWords * s + lane] = 0u;
    if (nb > W.nb_cap) {
        if (lane == 0) { prof_all[s].status = SLHIP_SETTLE_REFUSED_BODIES; H->status = 1; }
        return;
    }
    for (int i = lane; i < nb; i += 64) {
        int4* z = reinterpret_cast<int4*>(W.pp + (size_t)s * W.nb_cap + i);
        z[0] = make_int4(0, 0, 0, 0); z[1] = make_int4(0, 0, 0, 0);
    }
    // serial over bodies / hulls (a few hundred at most)
    int n_lh = 0;
    bool fits = true;
    for (int i = 0; i < nb && fits; ++i) {
        const int h0 = (int)bodies[i].hull_begin, h1 = (int)bodies[i].hull_end;
        if (lane == 0) body_lh[i] = n_lh;
        if (h1 - h0 > kMaxHullsPerBody || n_lh + (h1 - h0) > W.lh_cap) { fits = false; break; }
        for (int h = h0 + lane; h < h1; h += 64) {
            HullRef r;
            r.src = (int)hulls[h].vtx_begin;
            r.count = (int)hulls[h].vtx_count;
            r.sc = V(hulls[h].sphere[0], hulls[h].sphere[1], hulls[h].sphere[2]);
            r.sr = hulls[h].sphere[3];
            lh[n_lh + (h - h0)] = r;
        }
        n_lh += h1 - h0;
    }
    if (!fits || n_lh > 65535) {
        if (lane == 0) { prof_all[s].status = SLHIP_SETTLE_REFUSED_HULLS; H->status = 1; }
        return;
    }
    if (lane == 0) {
        body_lh[nb] = n_lh;
        prof_all[s].status = 0;
        H->status = 0;
        H->n_hp = 0; H->n_groups = 0; H->n_plane_groups = 0; H->n_active = 0; H->n_active_before_pairs = 0; H->ncol = 0;
        H->n_hulls = n_lh;
    }
    {
        const unsigned n = pc.hashed ? pc.stride : (unsigned)(n_lh * n_lh);
        if (n <= pc.stride) {
            int4* z = pc.base + (size_t)s * pc.stride;
            for (unsigned k = lane; k < n; k += 64) z[k] = make_int4(0, 0, 0, 0);
        }
    }
}

// LDS of k_w_begin: bodies, local hull table, hull offsets, the plane phase's band cache, the near-plane list
struct BeginLds { int off_wb, off_lh, off_body_lh, off_band, off_plist, total; };
__host__ __device__ inline BeginLds begin_layout(int nb_cap, int lh_cap)
{
    BeginLds L;
    int o = 0;
    auto take = [&](int bytes) { const int r = o; o += (bytes + 15) & ~15; return r; };
    L.off_wb = take(nb_cap * (int)sizeof(WBody));
    L.off_lh = take(lh_cap * (int)sizeof(HullRef));
    L.off_body_lh = take((nb_cap + 1) * 4);
    L.off_band = take(4 * kBandCap * (int)sizeof(BandPt));
    L.off_plist = take(64);
    L.total = o;
    return L;
}

// ---- (a) load + integrate forces, (b) table contacts, (c) broadphase ------------------------------------
// One scene, by one wave.  kFileWork: the scene's candidate pairs join the step's global work lists (the lockstep pipeline); the
// persistent kernel walks the scene's own list instead.
template <bool kFileWork>
__device__ __forceinline__ void begin_scene(char* smem, const int s, const unsigned n_scenes, const slhip_settle_scene* __restrict__ scenes,
                                            slhip_body* bodies_all, const slhip_hull* __restrict__ hulls, const float* __restrict__ hull_verts,
                                            const slhip_settle_params& prm, const WideBufs& W, const BeginLds& L, DriveAcc* drive_all, unsigned step)
{
    const int lane = threadIdx.x;
    WideHdr* H = W.hdr + s;
    if (H->status != 0) return;
    WBody* wb = reinterpret_cast<WBody*>(smem + L.off_wb);
    HullRef* lh = reinterpret_cast<HullRef*>(smem + L.off_lh);
    int* body_lh = reinterpret_cast<int*>(smem + L.off_body_lh);
    BandPt* band = reinterpret_cast<BandPt*>(smem + L.off_band);
    unsigned char* plist = reinterpret_cast<unsigned char*>(smem + L.off_plist);
    const float4* gv = reinterpret_cast<const float4*>(hull_verts);
    const f3* hv = reinterpret_cast<const f3*>(hull_verts);   // never read: every HullRef of this pipeline points into the global pool
    const slhip_settle_scene sc = scenes[s];
    slhip_body* bodies = bodies_all + sc.body_begin;
    const int nb = (int)(sc.body_end - sc.body_begin);
    const float dt = prm.dt;
    DriveAcc* drv = drive_all + (size_t)s * W.nb_cap;
    Contact* ac = W.ac + (size_t)s * W.c_cap;
    Group* groups = W.groups + (size_t)s * W.g_cap;
    HullPair* hp = W.hp + (size_t)s * W.p_cap;
    const int c_cap = W.c_cap, p_cap = W.p_cap;

    for (int k = lane; k <= nb; k += 64) body_lh[k] = W.body_lh[(size_t)s * (W.nb_cap + 1) + k];
    __syncthreads();
    wave_copy_words(lh, W.lh + (size_t)s * W.lh_cap, body_lh[nb] * (int)sizeof(HullRef), lane);
    // (a) load, integrate forces
    for (int i = lane; i < nb; i += 64) {
        load_body(bodies[i], wb[i]);
        update_world_inertia(bodies[i], wb[i]);
        if (wb[i].dynamic) {
            // stabilisation: a settling body feels a share of gravity (oracle step_scene (a))
            wb[i].v = madd(wb[i].v, V(prm.gravity[0], prm.gravity[1], prm.gravity[2]), dt * (1.0f - bodies[i].stab[1]));
            float damp = 1.0f - prm.angular_damping * dt;
            if (damp < 0.0f) damp = 0.0f;
            wb[i].w = scale(wb[i].w, damp);
        }
        if (bodies[i].drive_flags & 1u) {
            DriveAcc z;
            z.dl[0] = z.dl[1] = z.dl[2] = z.da[0] = z.da[1] = z.da[2] = 0.0f;
            drv[i] = z;
        }
    }
    __syncthreads();

    int n_groups = 0, n_active = 0;
    // (b) table contacts, groups + contacts appended in body order (see k_settle)
    if (sc.has_plane) {
        int off_run = n_active;
        for (int base = 0; base < nb; base += 64) {
            const int i = base + lane;
            bool pass = false;
            if (i < nb && wb[i].dynamic) {
                const v3 ci = add(m3_mul(wb[i].R, V(bodies[i].bsphere[0], bodies[i].bsphere[1], bodies[i].bsphere[2])), wb[i].t);
                const float vz = wb[i].v.z < 0.0f ? -wb[i].v.z * dt : 0.0f;
                pass = !(ci.z - bodies[i].bsphere[3] - sc.plane_z > prm.contact_offset + vz);
            }
            const int rank = compact_slot(pass, 0);
            const int n_pass = __popcll(__ballot(pass));
            if (pass) plist[rank] = (unsigned char)lane;
            __syncthreads();
            const int sg = lane >> 4, sl = lane & 15;
            for (int r0 = 0; r0 < n_pass; r0 += 4) {
                const bool on = r0 + sg < n_pass;
                const int bi = on ? base + (int)plist[r0 + sg] : 0;
                RawContacts rc;
                rc.count = 0;
                int ids[4] = {0, 0, 0, 0};
                if (on) {
                    const float vz = wb[bi].v.z < 0.0f ? -wb[bi].v.z * dt : 0.0f;
                    plane_contacts_sg16(wb[bi], lh, hv, gv, body_lh[bi], body_lh[bi + 1], sc.plane_z,
                                        prm.contact_offset + vz, band + sg * kBandCap, sg, sl, rc, ids);
                }
                // rows of the patch in the list: its centre row (three or four points: oracle patch_centre) at the head, then the points
                const int lead = rc.count >= 3 ? 1 : 0;
                const int rows = rc.count + lead;
                const int c0 = __shfl(rows, 0, 64), c1 = __shfl(rows, 16, 64), c2 = __shfl(rows, 32, 64);
                const int c3 = __shfl(rows, 48, 64);
                const int off = off_run + (sg > 0 ? c0 : 0) + (sg > 1 ? c1 : 0) + (sg > 2 ? c2 : 0);
                if (on) {
                    // the body's table contacts of the previous step: a vertex that was one of them starts from its impulse
                    PlanePM* ppm = W.pp + (size_t)s * W.nb_cap + bi;
                    const int4 q0 = reinterpret_cast<const int4*>(ppm)[0], q1 = reinterpret_cast<const int4*>(ppm)[1];
                    const bool prev_ok = (unsigned)q0.x == step - 1u;
                    const int pcount = prev_ok ? q0.y : 0, pc_off = q0.z;
                    const int my_id = sl == 0 ? ids[0] : sl == 1 ? ids[1] : sl == 2 ? ids[2] : ids[3];
                    if (lead && sl == 4 && off < c_cap) {
                        const float e = 0.5f * (bodies[bi].restitution + prm.plane_restitution);
                        v3 sra = V(0, 0, 0);
                        float ssp = 0.0f;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (q < rc.count) { sra = add(sra, sub(rc.pa[q], wb[bi].x)); ssp = ssp + rc.sep[q]; }
                        const float warm = (prev_ok && q1.w != 0) ? kWarmStart * (W.lnout + (size_t)s * c_cap + pc_off)[-1] : 0.0f;
                        fill_centre(&ac[off], bi, -1, rc.count, sra, V(0, 0, 0), ssp, rc.n, prm.rest_offset, e, warm);
                    }
                    if (sl < rc.count && off + lead + sl < c_cap) {
                        const float e = 0.5f * (bodies[bi].restitution + prm.plane_restitution);
                        const v3 pa = vsel(sl == 0, rc.pa[0], vsel(sl == 1, rc.pa[1], vsel(sl == 2, rc.pa[2], rc.pa[3])));
                        const float sp = sl == 0 ? rc.sep[0] : sl == 1 ? rc.sep[1] : sl == 2 ? rc.sep[2] : rc.sep[3];
                        float warm = 0.0f;
                        const float* lp = W.lnout + (size_t)s * c_cap + pc_off;
                        if (0 < pcount && q0.w == my_id) warm = kWarmStart * lp[0];
                        if (1 < pcount && q1.x == my_id) warm = kWarmStart * lp[1];
                        if (2 < pcount && q1.y == my_id) warm = kWarmStart * lp[2];
                        if (3 < pcount && q1.z == my_id) warm = kWarmStart * lp[3];
                        fill_contact(&ac[off + lead + sl], bi, -1, wb[bi], nullptr, pa, V(pa.x, pa.y, sc.plane_z), rc.n, sp,
                                     prm.rest_offset, e, sl == 0 && !lead, warm);
                    }
                    if (sl == 0) {
                        Group G;
                        G.a = (unsigned short)bi; G.b = (unsigned short)kNoBody;
                        G.begin = (unsigned short)min(off, c_cap); G.end = (unsigned short)min(off + rows, c_cap);
                        G.color = 0;
                        groups[n_groups + r0 + sg] = G;
                        const int written = max(0, min(rc.count, c_cap - off - lead));   // beyond the list's capacity: dropped (counted by k_w_finish)
                        // (c_off: the first POINT's impulse; the centre row's lies before it when the last word says there is one)
                        reinterpret_cast<int4*>(ppm)[0] = make_int4((int)step, written, off + lead, ids[0]);
                        reinterpret_cast<int4*>(ppm)[1] = make_int4(ids[1], ids[2], ids[3], (lead && off < c_cap) ? 1 : 0);
                    }
                }
                off_run += c0 + c1 + c2 + c3;
                __syncthreads();   // the band cache is reused by the next round
            }
            n_groups += n_pass;
        }
        n_active = off_run;          // what the table offers (k_w_finish clamps to the capacity and counts)
    }
    const int n_plane_groups = n_groups;

    // (c) broadphase: body pairs in (i<j) order -> hull pairs, ballot-compacted in order
    int n_hp = 0, hp_found = 0, g_overflow = 0;
    {
        const int n_pairs = nb * (nb - 1) / 2;
        for (int base = 0; base < n_pairs; base += 64) {
            const int p = base + lane;
            bool pass = false;
            int pi = 0, pj = 0;
            if (p < n_pairs) {
                int rem = p, row = nb - 1;
                while (rem >= row) { rem -= row; ++pi; --row; }
                pj = pi + 1 + rem;
                if (wb[pi].dynamic || wb[pj].dynamic) {
                    const v3 ci = add(m3_mul(wb[pi].R, V(bodies[pi].bsphere[0], bodies[pi].bsphere[1], bodies[pi].bsphere[2])), wb[pi].t);
                    const v3 cj = add(m3_mul(wb[pj].R, V(bodies[pj].bsphere[0], bodies[pj].bsphere[1], bodies[pj].bsphere[2])), wb[pj].t);
                    const v3 dv = sub(wb[pi].v, wb[pj].v);
                    const float margin = 2.0f * prm.contact_offset + sqrtf(dot(dv, dv)) * dt;
                    const v3 d = sub(ci, cj);
                    const float rr = bodies[pi].bsphere[3] + bodies[pj].bsphere[3] + margin;
                    pass = !(dot(d, d) > rr * rr);
                }
            }
            unsigned long long mask = __ballot(pass);
            while (mask) {
                const int src = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int i = __shfl(pi, src, 64), j = __shfl(pj, src, 64);
                const int la0 = body_lh[i], na = body_lh[i + 1] - la0;
                const int lb0 = body_lh[j], nbh = body_lh[j + 1] - lb0;
                const unsigned ga0 = bodies[i].hull_begin, gb0 = bodies[j].hull_begin;
                const v3 dv = sub(wb[i].v, wb[j].v);
                const float margin = 2.0f * prm.contact_offset + sqrtf(dot(dv, dv)) * dt;
                const int first = n_hp;
                const int combos = na * nbh;
                for (int cb = 0; cb < combos; cb += 64) {
                    const int q = cb + lane;
                    bool ok = false;
                    int a = 0, b = 0;
                    if (q < combos) {
                        a = q / nbh; b = q % nbh;
                        const HullRef& A = lh[la0 + a];
                        const HullRef& B = lh[lb0 + b];
                        const v3 ca = add(m3_mul(wb[i].R, A.sc), wb[i].t);
                        const v3 cbw = add(m3_mul(wb[j].R, B.sc), wb[j].t);
                        const v3 dd = sub(ca, cbw);
                        const float r2 = A.sr + B.sr + margin;
                        ok = !(dot(dd, dd) > r2 * r2);
                        if (ok) ok = aabb_overlap(wb[i], hulls[ga0 + a], wb[j], hulls[gb0 + b], margin);
                    }
                    const int slot = compact_slot(ok, n_hp);
                    if (ok && slot < p_cap) hp[slot] = hp_pack(i, j, a, b);
                    const int n_ok = (int)__popcll(__ballot(ok));
                    hp_found += n_ok;
                    n_hp = min(n_hp + n_ok, p_cap);      // beyond the list's capacity: dropped in list order, counted
                }
                if (n_hp > first && n_groups >= W.g_cap) {      // no room for another group (wide_g_cap): the body pair's hull pairs are dropped, counted
                    g_overflow = 1;
                    n_hp = first;
                }
                if (n_hp > first) {
                    if (lane == 0) {
                        Group G;
                        G.a = (unsigned short)i; G.b = (unsigned short)j;
                        G.begin = 0; G.end = 0;   // contact range: filled in by k_w_finish
                        G.color = 0;
                        groups[n_groups] = G;
                    }
                    ++n_groups;
                }
            }
        }
    }
    __syncthreads();
    wave_copy_words(W.wb + (size_t)s * W.nb_cap, wb, nb * (int)sizeof(WBody), lane);
    // the scene's candidate pairs join the step's global list (any order: every pair writes its own result slot)
    if (kFileWork && n_hp > 0) {
        // size class of every pair, counted, then one reservation per class and scene
        const size_t region = (size_t)n_scenes * p_cap;
        int cnt0 = 0, cnt1 = 0, cnt2 = 0;
        for (int k0 = 0; k0 < n_hp; k0 += 64) {
            const int k = k0 + lane;
            int cls = -1;
            if (k < n_hp) {
                const HullPair e = hp[k];
                const int m = max(lh[body_lh[hp_ba(e)] + hp_ha(e)].count, lh[body_lh[hp_bb(e)] + hp_hb(e)].count);
                cls = m <= 16 ? 0 : m <= 32 ? 1 : 2;
            }
            cnt0 += (int)__popcll(__ballot(cls == 0)); cnt1 += (int)__popcll(__ballot(cls == 1)); cnt2 += (int)__popcll(__ballot(cls == 2));
        }
        unsigned base = 0u;
        if (lane < 3) {
            const int c = lane == 0 ? cnt0 : lane == 1 ? cnt1 : cnt2;
            if (c > 0) base = atomicAdd(&W.work_count[8 + lane], (unsigned)c);
        }
        unsigned run0 = (unsigned)__shfl((int)base, 0, 64), run1 = (unsigned)__shfl((int)base, 1, 64), run2 = (unsigned)__shfl((int)base, 2, 64);
        for (int k0 = 0; k0 < n_hp; k0 += 64) {
            const int k = k0 + lane;
            int cls = -1;
            if (k < n_hp) {
                const HullPair e = hp[k];
                const int m = max(lh[body_lh[hp_ba(e)] + hp_ha(e)].count, lh[body_lh[hp_bb(e)] + hp_hb(e)].count);
                cls = m <= 16 ? 0 : m <= 32 ? 1 : 2;
            }
            const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2);
            const unsigned long long below = (1ull << lane) - 1ull;
            const unsigned entry = ((unsigned)s << W.pair_bits) | (unsigned)k;
            if (cls == 0) W.work[run0 + (unsigned)__popcll(m0 & below)] = entry;
            if (cls == 1) W.work[region + run1 + (unsigned)__popcll(m1 & below)] = entry;
            if (cls == 2) W.work[2 * region + run2 + (unsigned)__popcll(m2 & below)] = entry;
            run0 += (unsigned)__popcll(m0); run1 += (unsigned)__popcll(m1); run2 += (unsigned)__popcll(m2);
        }
    }
    if (lane == 0) {
        H->n_hp = n_hp; H->n_groups = n_groups; H->n_plane_groups = n_plane_groups;
        H->n_active_before_pairs = n_active; H->n_active = n_active;
        H->hp_overflow = hp_found > p_cap ? 1 : 0; H->hp_found = hp_found; H->g_overflow = g_overflow;
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void k_w_begin(const slhip_settle_scene* __restrict__ scenes, slhip_body* bodies_all,
                                               const slhip_hull* __restrict__ hulls, const float* __restrict__ hull_verts,
                                               slhip_settle_params prm, WideBufs W, BeginLds L, DriveAcc* drive_all, unsigned step)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (before the early return: scene 0 may be a refused one, and the classes must be cleared all the same)
    if (blockIdx.x == 0) for (int k = threadIdx.x; k < kLptWords; k += 64) W.lpt_count[k] = 0u;   // the previous step's k_w_solve has read them
    begin_scene<true>(smem, (int)blockIdx.x, gridDim.x, scenes, bodies_all, hulls, hull_verts, prm, W, L, drive_all, step);
}

// ---- (d1) main GJK: lane = hull pair of ANY scene ------------------------------------------------------
// Two passes over compacted work lists.  63 % of the runs end in their first iteration (the cached simplex still separates the
// pair beyond the margin), 13 % in the second, the longest take nine (tools/solver_stats.py) -- with 64 pairs of one scene per
// wave a wave ran as long as its slowest pair with 7 of 64 lanes busy.  Pass 1 gives every pair ONE iteration and lists the
// pairs that are not done; pass 2 runs those from the start (same inputs, same function: the same result as an uninterrupted
// run), now with waves full of pairs that all iterate.  A finished pair writes its result slot, its cache entry and -- if it is
// a contact pair -- its bit of the scene's mask (atomic OR; k_w_begin cleared the masks).
__device__ __forceinline__ int gjk_work_item(unsigned e_work, const float* __restrict__ hull_verts, const slhip_settle_params& prm,
                                              const WideBufs& W, const PairCache& pc, int max_iter,
                                              unsigned step, unsigned n_scenes, bool& unfinished)
{
    const int s = (int)(e_work >> W.pair_bits), k = (int)(e_work & ((1u << W.pair_bits) - 1u));
    WideHdr* H = W.hdr + s;
    const float4* gv = reinterpret_cast<const float4*>(hull_verts);
    const WBody* wb = W.wb + (size_t)s * W.nb_cap;
    const HullRef* lh = W.lh + (size_t)s * W.lh_cap;
    const int* body_lh = W.body_lh + (size_t)s * (W.nb_cap + 1);
    MainResult mr;
    mr.type = 0; mr.dist = 0.0f;
    mr.n = V(0, 0, 0); mr.pa = V(0, 0, 0); mr.pb = V(0, 0, 0);
    mr.seed.n = 0; mr.seed.i0 = mr.seed.i1 = mr.seed.i2 = 0;
    const HullPair e = W.hp[(size_t)s * W.p_cap + k];
    const int ba = hp_ba(e), bb = hp_bb(e);
    const WBody wa = wb[ba], wbb = wb[bb];
    const v3 dv = sub(wa.v, wbb.v);
    const float margin = 2.0f * prm.contact_offset + sqrtf(dot(dv, dv)) * prm.dt;
    const int la = body_lh[ba] + hp_ha(e), lb = body_lh[bb] + hp_hb(e);
    GjkSeed cached;
    cached.n = 0; cached.i0 = cached.i1 = cached.i2 = 0;
    // pair cache (oracle scene_ws.cache + pm): what the previous step left for this pair, if it listed the pair at all
    const int n_hulls = H->n_hulls;
    const int4* slot_p = pair_cache_slot(pc, s, n_hulls, la, lb, step - 1u, false);
    bool prev_ok = false, prev_filed = false;
    int prev_slot = 0;
    if (slot_p) {
        const int4 q = *slot_p;
        if (((unsigned)q.x >> 3) == ((step - 1u) & 0x1fffffffu)) {
            cached.n = q.x & 3; cached.i0 = sv_unpack(q.y & 0xffff); cached.i1 = sv_unpack((q.y >> 16) & 0xffff); cached.i2 = sv_unpack(q.z & 0xffff);
            // the pair's manifold of the previous step, if that step filed one (its centre row's impulse is carried even when the
            // list's capacity left it no point: oracle hull_pair_contacts, prev.lc), and whether it has points to refresh
            if (((q.x >> 2) & 1) != 0) {
                prev_slot = (int)((unsigned)q.z >> 16);
                prev_filed = true;
                prev_ok = W.pm[((size_t)((step - 1u) & 1u) * n_scenes + s) * W.p_cap + prev_slot].count > 0;
            }
        }
    }
    const HullRef ha = lh[la], hb = lh[lb];
    const bool rewrite = pair_main(wa, wbb, ha, hb, reinterpret_cast<const f3*>(hull_verts), gv, margin, cached, mr, max_iter, &unfinished);
    if (unfinished) return 0;
    if (int4* slot_c = pair_cache_slot(pc, s, n_hulls, la, lb, step, true)) {
        const GjkSeed w = rewrite ? mr.seed : cached;        // an overlap keeps the old simplex
        const int4 e = make_int4(cache_x(w.n, mr.type != 0, step), sv_pack(w.i0) | (sv_pack(w.i1) << 16), sv_pack(w.i2) | (k << 16), 0);
        if (pc.hashed) { slot_c->x = e.x; slot_c->y = e.y; slot_c->z = e.z; }      // (w is the key)
        else *slot_c = e;
    }
    if (mr.type != 0) {
        // the manifold the previous step left: its points in the new poses, parked in the pair's stage slots.  It stays (type 3)
        // unless a point went or the closest points are deeper than all of it; a new pair and a lost manifold are built by
        // k_w_manifold (type 1)
        int no = 0;
        bool lost = true;
        if (prev_ok) {
            const PM prev = W.pm[((size_t)((step - 1u) & 1u) * n_scenes + s) * W.p_cap + prev_slot];
            const float* lnout = W.lnout + (size_t)s * W.c_cap;
            no = refresh_manifold(mr, prev, prev.c_off >= 0 ? lnout + prev.c_off : kNoImpulse, wa, wbb, margin, prm.contact_offset,
                                  W.stage + ((size_t)s * W.p_cap + k) * 4, lost);
        }
        mr.type = lost ? 1 : 3;
        mr.seed.n = prev_slot; mr.seed.i0 = prev_filed ? 1 : 0; mr.seed.i1 = no; mr.seed.i2 = 0;
    }
    W.mr[(size_t)s * W.p_cap + k] = mr;
    return mr.type;
}

// The threads of a 256-thread block append `e` to work list 1 where `p1` holds and to list 2 where `p2` holds: ONE 64-bit atomic
// per block for both lists (list 1's length in the low word of work_count[2..3], list 2's in the high word).  Thousands of
// waves bumping one address at the same moment queue up behind each other -- one atomic per wave and list cost the first pass
// 0.12 ms of its 0.29.
__device__ __forceinline__ void work_push2(const WideBufs& W, unsigned list_stride, bool p1, bool p2, unsigned e)
{
    __shared__ unsigned s_cnt[2][4];
    __shared__ unsigned s_base[2];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long m1 = __ballot(p1), m2 = __ballot(p2);
    if (lane == 0) { s_cnt[0][wv] = (unsigned)__popcll(m1); s_cnt[1][wv] = (unsigned)__popcll(m2); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t1 = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        const unsigned t2 = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
        unsigned long long old = 0ull;
        if ((t1 | t2) != 0u)
            old = atomicAdd(reinterpret_cast<unsigned long long*>(W.work_count + 2), (unsigned long long)t1 | ((unsigned long long)t2 << 32));
        s_base[0] = (unsigned)old; s_base[1] = (unsigned)(old >> 32);
    }
    __syncthreads();
    unsigned b1 = s_base[0], b2 = s_base[1];
    for (unsigned w = 0; w < wv; ++w) { b1 += s_cnt[0][w]; b2 += s_cnt[1][w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (p1) W.work[3 * (size_t)list_stride + b1 + (unsigned)__popcll(m1 & below)] = e;
    if (p2) W.work[4 * (size_t)list_stride + b2 + (unsigned)__popcll(m2 & below)] = e;
    __syncthreads();   // the counts are rewritten by the block's next pass
}

// Single waves: next to the render stream's kernels a 256-thread block waits until FOUR SIMDs have 151 registers free at the same
// moment (0.18 ms alone became 0.95 ms in the pipeline); a wave needs one.  The two list appends of a wave are ONE 64-bit atomic.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void k_w_gjk_first(const float* __restrict__ hull_verts, slhip_settle_params prm, WideBufs W,
                                                   PairCache pc, unsigned list_stride, unsigned step, unsigned n_scenes)
{
    const unsigned lane = threadIdx.x;
    const unsigned n0 = W.work_count[8], n1 = W.work_count[9], n2 = W.work_count[10];
    const unsigned total = n0 + n1 + n2;                 // list 0: the three size classes one after the other
    for (unsigned i0 = blockIdx.x * 64u; i0 < total; i0 += gridDim.x * 64u) {
        const unsigned i = i0 + lane;
        bool unfinished = false;
        unsigned e = 0u;
        int type = 0;
        if (i < total) {
            e = i < n0 ? W.work[i] : i < n0 + n1 ? W.work[(size_t)list_stride + (i - n0)] : W.work[2 * (size_t)list_stride + (i - n0 - n1)];
            type = gjk_work_item(e, hull_verts, prm, W, pc, 1, step, n_scenes, unfinished);
        }
        const bool p2 = type == 1;   // the pairs whose manifold is built in this step
        const unsigned long long m1 = __ballot(unfinished), m2 = __ballot(p2);
        if ((m1 | m2) != 0ull) {
            unsigned long long old = 0ull;
            if (lane == 0)
                old = atomicAdd(reinterpret_cast<unsigned long long*>(W.work_count + 2),
                                (unsigned long long)__popcll(m1) | ((unsigned long long)__popcll(m2) << 32));
            const unsigned b1 = (unsigned)__shfl((int)(unsigned)old, 0, 64), b2 = (unsigned)__shfl((int)(unsigned)(old >> 32), 0, 64);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (unfinished) W.work[3 * (size_t)list_stride + b1 + (unsigned)__popcll(m1 & below)] = e;
            if (p2) W.work[4 * (size_t)list_stride + b2 + (unsigned)__popcll(m2 & below)] = e;
        }
    }
}

// second pass: single waves (a block would wait for its slowest wave, and these runs differ by up to eight iterations); the
// contact pairs found here join list 2 with one 32-bit atomic per wave on the high word of the pair of counters
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void k_w_gjk_rest(const float* __restrict__ hull_verts, slhip_settle_params prm, WideBufs W,
                                                  PairCache pc, unsigned list_stride, unsigned step, unsigned n_scenes)
{
    const unsigned lane = threadIdx.x;
    const unsigned total = W.work_count[2];
    for (unsigned i0 = blockIdx.x * 64u; i0 < total; i0 += gridDim.x * 64u) {
        const unsigned i = i0 + lane;
        bool unfinished = false;
        unsigned e = 0u;
        int type = 0;
        if (i < total) {
            e = W.work[3 * (size_t)list_stride + i];
            type = gjk_work_item(e, hull_verts, prm, W, pc, kGjkMaxIter, step, n_scenes, unfinished);
        }
        const bool push = type == 1;
        const unsigned long long m = __ballot(push);
        if (m != 0ull) {
            unsigned base = 0u;
            if (lane == 0) base = atomicAdd(&W.work_count[3], (unsigned)__popcll(m));
            base = (unsigned)__shfl((int)base, 0, 64);
            if (push) W.work[4 * (size_t)list_stride + base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = e;
        }
    }
}

// ---- (d2) face manifolds: 8 lanes = one contact pair of ANY scene that is new or lost a point, eight pairs per wave pass ----
// (oracle face_manifold: same expressions, every selection an arg-min / arg-max over (value, candidate number).)  The lanes of a
// pair split the hulls' vertices eight each for the support features, hold the two polygons redundantly (a winner's coordinates
// come from the lane that holds the vertex), and own the candidates
//     lane l < 4: the kept point l (candidate l);  lane 4: the closest points (candidate 4);
//     lane l: A's polygon vertex l in B's polygon (candidate 5 + l) and B's vertex l in A's (candidate 13 + l);
//     lane l: the crossings of A's edge l with B's eight edges (candidates 21 + 8 l + j).
// Reductions across the 8 lanes are three DPP steps (lane ^ 1, lane ^ 2 within the quad, then the half row mirrored).
template <int CTRL>
__device__ __forceinline__ float sg8_dpp(float v) { return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true)); }
template <int CTRL>
__device__ __forceinline__ int sg8_dpp(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ float sg8_min(float v)
{
    v = fminf(v, sg8_dpp<0xB1>(v)); v = fminf(v, sg8_dpp<0x4E>(v)); v = fminf(v, sg8_dpp<0x141>(v));
    return v;
}
__device__ __forceinline__ float sg8_max(float v)
{
    v = fmaxf(v, sg8_dpp<0xB1>(v)); v = fmaxf(v, sg8_dpp<0x4E>(v)); v = fmaxf(v, sg8_dpp<0x141>(v));
    return v;
}
template <int CTRL>
__device__ __forceinline__ void sg8_argmin_step(float& val, int& idx)
{
    const float ov = sg8_dpp<CTRL>(val);
    const int oi = sg8_dpp<CTRL>(idx);
    if (ov < val || (ov == val && oi < idx)) { val = ov; idx = oi; }
}
// the (value, number) minimum of the pair's eight lanes, in every lane (a total order: the combine is associative and commutative)
__device__ __forceinline__ void sg8_argmin(float& val, int& idx)
{
    sg8_argmin_step<0xB1>(val, idx);    // quad_perm [1,0,3,2]
    sg8_argmin_step<0x4E>(val, idx);    // quad_perm [2,3,0,1]
    sg8_argmin_step<0x141>(val, idx);   // row_half_mirror
}
constexpr int kFmNone = 0x7fffffff;
// A value the optimiser must treat as a plain register value: a select between two array elements (`c ? P.u[k] : Q.u[k]`) is
// otherwise folded into a load through a selected POINTER, which pins the polygons in scratch memory.
__device__ __forceinline__ float fm_val(float x) { asm("" : "+v"(x)); return x; }
// words of a pair's strip of LDS in k_w_manifold: u, w, h of a hull's 64 vertex slots.  (Round 6 measured a pitch of 200 words -- the
// eight pairs of a wave then cover the 64 banks once where at 192 they meet in the same eight -- : 0.328 ms per launch either way.)
constexpr int kFmStrip = 192;
struct FmPoly { float u[8], w[8], h[8]; };
struct FmCand { float u, w, ha, hb, sep; int id; bool ok; };

// support feature of one hull along n: `lowest` = the side facing down the normal (A), else up (B)
__device__ __forceinline__ void fm_feature(const float4* __restrict__ gv, const HullRef& H, const m3& R, v3 t, v3 n, v3 t1, v3 t2,
                                           bool lowest, float band, int sl, float* __restrict__ lds, FmPoly& P)
{
    const v3 nl = m3_tmul(R, n), l1 = m3_tmul(R, t1), l2 = m3_tmul(R, t2);
    const float on = dot(t, n), o1 = dot(t, t1), o2 = dot(t, t2);
    const float4* v = gv + H.src;
    float hh[8], uu[8], ww[8];
    float lo = kInf, hi = -kInf;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = sl + 8 * k;
        const float4 q = v[min(i, H.count - 1)];
        const v3 p = V(q.x, q.y, q.z);
        hh[k] = dot(p, nl) + on; uu[k] = dot(p, l1) + o1; ww[k] = dot(p, l2) + o2;
        if (i < H.count) { lo = fminf(lo, hh[k]); hi = fmaxf(hi, hh[k]); }
    }
    lo = sg8_min(lo); hi = sg8_max(hi);
    const float ext = lowest ? lo : hi;
    if (band > kFmBandExtent * (hi - lo)) band = kFmBandExtent * (hi - lo);
    float best[8];
    int bi[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) { best[d] = -kInf; bi[d] = kFmNone; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = sl + 8 * k;
        const bool in = i < H.count && !(lowest ? hh[k] > ext + band : hh[k] < ext - band);
        const float u = uu[k], w = ww[k];
        float sc[8];
        sc[0] = u; sc[1] = u + w; sc[2] = w; sc[3] = w - u;
        sc[4] = -sc[0]; sc[5] = -sc[1]; sc[6] = -sc[2]; sc[7] = -sc[3];
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (in && (bi[d] == kFmNone || sc[d] > best[d])) { best[d] = sc[d]; bi[d] = i; }
    }
    // arg-max over the pair's lanes: the higher score, the lower vertex number among equals (a lane without a vertex in the band
    // offers -inf / none); the winners' coordinates go through the pair's strip of LDS (three floats per vertex)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = sl + 8 * k;
        lds[i] = uu[k]; lds[64 + i] = ww[k]; lds[128 + i] = hh[k];
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        float nv = -best[d];
        int ni = bi[d];
        sg8_argmin(nv, ni);
        P.u[d] = lds[ni]; P.w[d] = lds[64 + ni]; P.h[d] = lds[128 + ni];
    }
    __syncthreads();
}

// plane of a polygon (Newell, relative to slot 0) through the mean of its slots; nh = twice its area
struct FmPlane { float nu, nw, nh, cu, cw, ch; };
__device__ __forceinline__ FmPlane fm_plane(const FmPoly& P)
{
    float nu = 0.0f, nw = 0.0f, nh = 0.0f, su = 0.0f, sw = 0.0f, sh = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int k1 = (k + 1) & 7;
        const float au = P.u[k] - P.u[0], aw = P.w[k] - P.w[0], ah = P.h[k] - P.h[0];
        const float bu = P.u[k1] - P.u[0], bw = P.w[k1] - P.w[0], bh = P.h[k1] - P.h[0];
        nu = nu + (aw * bh - ah * bw);
        nw = nw + (ah * bu - au * bh);
        nh = nh + (au * bw - aw * bu);
        su = su + au; sw = sw + aw; sh = sh + ah;
    }
    FmPlane F;
    F.nu = nu; F.nw = nw; F.nh = nh; F.cu = su * 0.125f; F.cw = sw * 0.125f; F.ch = sh * 0.125f;
    return F;
}
// is (u, w) inside polygon Q (a polygon without area holds nothing), and Q's plane height there
__device__ __forceinline__ bool fm_inside(const FmPoly& Q, const FmPlane& F, float u, float w, float& hq)
{
    bool in = F.nh > kFmAreaMin;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int k1 = (k + 1) & 7;
        const float eu = Q.u[k1] - Q.u[k], ew = Q.w[k1] - Q.w[k];
        const float cr = eu * (w - Q.w[k]) - ew * (u - Q.u[k]);
        if (cr < -kFmInsideTol) in = false;
    }
    const float du = (u - Q.u[0]) - F.cu, dw = (w - Q.w[0]) - F.cw;
    hq = (Q.h[0] + F.ch) - (F.nu * du + F.nw * dw) / F.nh;
    return in;
}

#ifndef SLHIP_FM_WAVES
#define SLHIP_FM_WAVES 2
#endif
constexpr int kFmCands = 11;
// the lane's value of the candidate numbered `id` (the owner lane's is the one that counts)
template <class F>
__device__ __forceinline__ float fm_mine(const FmCand (&c)[kFmCands], int id, F f)
{
    float r = fm_val(f(c[0]));
#pragma unroll
    for (int q = 1; q < kFmCands; ++q) r = c[q].id == id ? fm_val(f(c[q])) : r;
    return r;
}
// The manifolds of the pairs `list[first .. total)` taken eight at a time with a stride (a wave = eight pairs of eight lanes).
__device__ __forceinline__ void manifold_items(const float* __restrict__ hull_verts, const slhip_settle_params& prm, const WideBufs& W,
                                               const unsigned* __restrict__ list, const unsigned total, const unsigned first, const unsigned stride,
                                               float (*s_uwh)[kFmStrip])
{
    const unsigned lane = threadIdx.x;
    const int sg = (int)(lane >> 3), sl = (int)(lane & 7u);
    const float4* gv = reinterpret_cast<const float4*>(hull_verts);
    for (unsigned it0 = first; it0 < total; it0 += stride) {
        // (every lane of the wave goes through the same instructions: the cross-lane steps need all eight lanes of a pair, and
        // a group beyond the list's end works on the list's last pair without writing)
        const bool live = it0 + (unsigned)sg < total;
        const unsigned item = live ? it0 + (unsigned)sg : total - 1u;
        const unsigned ew = list[item];
        const int s = (int)(ew >> W.pair_bits), kk = (int)(ew & ((1u << W.pair_bits) - 1u));
        const WBody* wb = W.wb + (size_t)s * W.nb_cap;
        const HullRef* lh = W.lh + (size_t)s * W.lh_cap;
        const int* body_lh = W.body_lh + (size_t)s * (W.nb_cap + 1);
        MainResult* mrp = W.mr + (size_t)s * W.p_cap + kk;
        StagePt* stage = W.stage + ((size_t)s * W.p_cap + kk) * 4;
        const HullPair e = W.hp[(size_t)s * W.p_cap + kk];
        const int bi = hp_ba(e), bj = hp_bb(e);
        const m3 Ra = wb[bi].R, Rb = wb[bj].R;
        const v3 ta = wb[bi].t, tb = wb[bj].t;
        const v3 dv = sub(wb[bi].v, wb[bj].v);
        const float margin = 2.0f * prm.contact_offset + sqrtf(dot(dv, dv)) * prm.dt;
        const HullRef ha = lh[body_lh[bi] + hp_ha(e)], hb = lh[body_lh[bj] + hp_hb(e)];
        const float radius = ha.sr <= hb.sr ? ha.sr : hb.sr;
        const float dup2 = 2.5e-3f * radius * radius;
        const v3 n = mrp->n, gpa = mrp->pa, gpb = mrp->pb;
        const float sep_new = mrp->dist;
        const int no = mrp->seed.i1;
        v3 t1, t2;
        tangents(n, &t1, &t2);

        FmPoly PA, PB;
        const float band = kFmBandOffsets * prm.contact_offset;
        fm_feature(gv, ha, Ra, ta, n, t1, t2, true, band, sl, s_uwh[sg], PA);
        fm_feature(gv, hb, Rb, tb, n, t1, t2, false, band, sl, s_uwh[sg], PB);
        const FmPlane FA = fm_plane(PA), FB = fm_plane(PB);

        // ---- the lane's candidates
        FmCand c[kFmCands];
        float imp0 = 0.0f;                 // impulse of the kept point (candidate 0 of lanes 0..3)
        v3 kqa = V(0, 0, 0), kqb = V(0, 0, 0);
        // [0] a kept point / the closest points
        {
            c[0].ok = sl < no;               // (the closest points: decided below)
            c[0].id = sl < 5 ? sl : kFmNone;
            v3 a = gpa;
            float sp = sep_new;
            if (sl < 4 && sl < no) {
                const StagePt t = stage[sl];
                a = t.qa; sp = t.sp; imp0 = __int_as_float(t.imp);
                kqa = t.qa; kqb = t.qb;
            }
            c[0].u = dot(a, t1); c[0].w = dot(a, t2); c[0].ha = dot(a, n);
            c[0].sep = sp; c[0].hb = c[0].ha - sp;
        }
        // hulls that overlap deeper than their support features reach have no face manifold: the kept points and the deepest points
        const bool deep = sep_new < -kFmDeepOffsets * prm.contact_offset;
        // the lane's vertex of either polygon, A's edge l
        float au0 = 0.0f, aw0 = 0.0f, ah0 = 0.0f, au1 = 0.0f, aw1 = 0.0f, ah1 = 0.0f, bu = 0.0f, bw = 0.0f, bh = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool m0 = k == sl, m1 = k == ((sl + 1) & 7);
            const float pu = fm_val(PA.u[k]), pw = fm_val(PA.w[k]), ph = fm_val(PA.h[k]);
            au0 = m0 ? pu : au0; aw0 = m0 ? pw : aw0; ah0 = m0 ? ph : ah0;
            au1 = m1 ? pu : au1; aw1 = m1 ? pw : aw1; ah1 = m1 ? ph : ah1;
            const float qu = fm_val(PB.u[k]), qw = fm_val(PB.w[k]), qh = fm_val(PB.h[k]);
            bu = m0 ? qu : bu; bw = m0 ? qw : bw; bh = m0 ? qh : bh;
        }
        // [1] A's vertex l inside B's polygon, [2] B's vertex l inside A's
        {
            float hq;
            const bool in = fm_inside(PB, FB, au0, aw0, hq);
            c[1].u = au0; c[1].w = aw0; c[1].ha = ah0; c[1].hb = hq; c[1].sep = 0.0f;
            c[1].ok = in && !deep; c[1].id = 5 + sl;
        }
        {
            float hq;
            const bool in = fm_inside(PA, FA, bu, bw, hq);
            c[2].u = bu; c[2].w = bw; c[2].ha = hq; c[2].hb = bh; c[2].sep = 0.0f;
            c[2].ok = in && !deep; c[2].id = 13 + sl;
        }
        // [3..10] crossings of A's edge l with B's edges 0 .. 7
        {
            const float eau = au1 - au0, eaw = aw1 - aw0;
            const float la = eau * eau + eaw * eaw;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int j1 = (j + 1) & 7;
                const float ebu = PB.u[j1] - PB.u[j], ebw = PB.w[j1] - PB.w[j];
                const float den = eau * ebw - eaw * ebu;
                const float lb = ebu * ebu + ebw * ebw;
                bool ok = den * den > kFmParallel2 * (la * lb);
                const float du = PB.u[j] - au0, dw = PB.w[j] - aw0;
                const float ss = (du * ebw - dw * ebu) / den, tt = (du * eaw - dw * eau) / den;
                ok = ok && ss >= 0.0f && ss <= 1.0f && tt >= 0.0f && tt <= 1.0f;
                c[3 + j].u = fmaf(ss, eau, au0); c[3 + j].w = fmaf(ss, eaw, aw0);
                c[3 + j].ha = fmaf(ss, ah1 - ah0, ah0);
                c[3 + j].hb = fmaf(tt, PB.h[j1] - PB.h[j], PB.h[j]);
                c[3 + j].sep = 0.0f;
                c[3 + j].ok = ok && !deep;
                c[3 + j].id = 21 + 8 * sl + j;
            }
        }
        // corners: a separation below the hulls' distance is an artefact of the plane fit; beyond the margin it is no contact
        float cmin = kInf;
        if (c[0].ok) cmin = c[0].sep;       // (lanes < no: kept points)
#pragma unroll
        for (int q = 1; q < kFmCands; ++q) {
            float sep = c[q].ha - c[q].hb;
            if (sep < sep_new) { sep = sep_new; c[q].hb = c[q].ha - sep; }
            c[q].sep = sep;
            if (sep > margin) c[q].ok = false;
            if (c[q].ok && sep < cmin) cmin = sep;
        }
        cmin = sg8_min(cmin);
        // the closest points join when nothing else is there, or when they are deeper than everything else
        const bool join = !(cmin < kInf) || sep_new < cmin - kFmDeeperOffsets * prm.contact_offset;
        if (sl == 4) c[0].ok = join;
        // a corner that coincides with a kept point or with the closest points is dropped
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float ku = __shfl(c[0].u, k, 8), kw = __shfl(c[0].w, k, 8), kh = __shfl(c[0].ha, k, 8);
            const bool kok = __shfl(c[0].ok ? 1 : 0, k, 8) != 0;
            if (__ballot(kok) == 0ull) continue;      // (no pair of the wave has this point)
#pragma unroll
            for (int q = 1; q < kFmCands; ++q) {
                const float du = c[q].u - ku, dw = c[q].w - kw, dh = c[q].ha - kh;
                if (kok && fmaf(dh, dh, fmaf(dw, dw, du * du)) < dup2) c[q].ok = false;
            }
        }
        // owner lane of candidate `id` (within the pair's 8 lanes) and the lane's value of a candidate it owns
        auto owner = [&](int id) -> int { return id < 5 ? id : id < 13 ? id - 5 : id < 21 ? id - 13 : (id - 21) >> 3; };
#define FM_MINE(id_, f_) fm_mine(c, (id_), [](const FmCand& x) { return x.f_; })
#define FM_FETCH(id_, f_) __shfl(FM_MINE(id_, f_), owner(id_), 8)
        // the deepest
        float v0 = kInf; int i0 = kFmNone;
#pragma unroll
        for (int q = 0; q < kFmCands; ++q)
            if (c[q].ok && (c[q].sep < v0 || (c[q].sep == v0 && c[q].id < i0))) { v0 = c[q].sep; i0 = c[q].id; }
        sg8_argmin(v0, i0);
        const float u0 = FM_FETCH(i0, u), w0 = FM_FETCH(i0, w), h0 = FM_FETCH(i0, ha), s0 = v0;
        // the farthest from it (not a duplicate of it), a metre of extra separation costing kDepthWeight metres of reach
        float v1 = kInf; int i1 = kFmNone;
#pragma unroll
        for (int q = 0; q < kFmCands; ++q) {
            const float du = c[q].u - u0, dw = c[q].w - w0, dh = c[q].ha - h0;
            const float d2 = fmaf(dh, dh, fmaf(dw, dw, du * du));
            const float score = -(sqrtf(d2) - kDepthWeight * (c[q].sep - s0));
            const bool cand = c[q].ok && c[q].id != i0 && !(d2 < dup2);
            if (cand && (i1 == kFmNone || score < v1 || (score == v1 && c[q].id < i1))) { v1 = score; i1 = c[q].id; }
        }
        sg8_argmin(v1, i1);
        int i2 = kFmNone, i3 = kFmNone;
        if (i1 != kFmNone) {     // (uniform over the pair's lanes)
            const float u1 = FM_FETCH(i1, u), w1 = FM_FETCH(i1, w);
            const float eu = u1 - u0, ew2 = w1 - w0;
            const float el = sqrtf(fmaf(ew2, ew2, eu * eu));
            float v2 = kInf, v3_ = kInf;
#pragma unroll
            for (int q = 0; q < kFmCands; ++q) {
                const float a = eu * (c[q].w - w0) - ew2 * (c[q].u - u0);
                const float pen = kDepthWeight * (c[q].sep - s0) * el;
                const bool cand = c[q].ok && c[q].id != i0 && c[q].id != i1;
                const float hi2 = -(a - pen), lo3 = a + pen;
                if (cand && a - pen > 0.0f && (i2 == kFmNone || hi2 < v2 || (hi2 == v2 && c[q].id < i2))) { v2 = hi2; i2 = c[q].id; }
                if (cand && a + pen < 0.0f && (i3 == kFmNone || lo3 < v3_ || (lo3 == v3_ && c[q].id < i3))) { v3_ = lo3; i3 = c[q].id; }
            }
            sg8_argmin(v2, i2);
            sg8_argmin(v3_, i3);
        }
        // the manifold, in the order deepest, farthest, area extremes: every point is written by the lane that owns it
        const int slot1 = 1, slot2 = 2, slot3 = i2 != kFmNone ? 3 : 2;
        const int nc = 1 + (i1 != kFmNone ? 1 : 0) + (i2 != kFmNone ? 1 : 0) + (i3 != kFmNone ? 1 : 0);
        auto slot_of = [&](int id) -> int { return id == i0 ? 0 : id == i1 ? slot1 : id == i2 ? slot2 : id == i3 ? slot3 : -1; };
        {
            const int sk = c[0].id == kFmNone ? -1 : slot_of(c[0].id);
            if (live && sk >= 0) {
                StagePt t;
                const bool kept = sl < 4;
                t.qa = vsel(kept, kqa, gpa); t.qb = vsel(kept, kqb, gpb); t.sp = c[0].sep; t.imp = kept ? __float_as_int(imp0) : 0;
                stage[sk] = t;
            }
        }
#pragma unroll
        for (int q = 1; q < kFmCands; ++q) {
            const int sk = c[q].ok ? slot_of(c[q].id) : -1;
            if (live && sk >= 0) {
                StagePt t;
                const v3 base = madd(scale(t1, c[q].u), t2, c[q].w);
                t.qa = madd(base, n, c[q].ha); t.qb = madd(base, n, c[q].hb); t.sp = c[q].sep; t.imp = 0;
                stage[sk] = t;
            }
        }
        if (live && sl == 0) mrp->seed.i1 = nc;
    }
#undef FM_MINE
#undef FM_FETCH
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SLHIP_FM_WAVES))) void k_w_manifold(const float* __restrict__ hull_verts, slhip_settle_params prm, WideBufs W,
                                                  unsigned list_stride)
{
    __shared__ float s_uwh[8][kFmStrip];                   // per pair: u, w, h of a hull's 64 vertex slots
    // contact pairs of all scenes whose manifold is built in this step
    manifold_items(hull_verts, prm, W, W.work + 4 * (size_t)list_stride, W.work_count[3], blockIdx.x * 8u, gridDim.x * 8u, s_uwh);
}

// bytes of LDS a scene's solve takes when everything it touches is resident (packed: sizes of THIS step, 16-byte aligned parts)
__host__ __device__ inline int solve_need(int nb, int n_groups, int ncol, int n_active)
{
    auto al = [](int b) { return (b + 15) & ~15; };
    return al(nb * (int)sizeof(SBody)) + al(n_groups * (int)sizeof(Group)) + al((n_groups + ncol + 2) * 2) + al(n_active * (int)sizeof(Contact));
}

// LDS of k_w_finish (the per-hull-pair lists -- group, kept contacts, offsets -- live in the scratch: a scene's pair list has no
// fixed size)
struct FinishLds { int off_wb, off_groups, off_gcnt, off_order, off_misc, off_hp, off_hp_off, off_hp_grp, total; };
constexpr int kFinishLdsPairs = 512;   // scenes with at most this many hull pairs in the step keep the per-pair lists in LDS
__host__ __device__ inline FinishLds finish_layout(int nb_cap, int g_cap)
{
    FinishLds L;
    int o = 0;
    auto take = [&](int bytes) { const int r = o; o += (bytes + 15) & ~15; return r; };
    L.off_wb = take(nb_cap * (int)sizeof(WBody));
    L.off_groups = take(g_cap * (int)sizeof(Group));
    L.off_gcnt = take(g_cap * 3 * 4);                       // per group: its contact pairs, the points they offer, its first hull pair
    L.off_order = take((2 * g_cap + 66) * 2);
    L.off_misc = take(nb_cap * 8 + nb_cap * 4 + nb_cap * 4 + 64);
    L.off_hp = take(kFinishLdsPairs * (int)sizeof(HullPair));
    L.off_hp_off = take((kFinishLdsPairs + 1) * 2);
    L.off_hp_grp = take(kFinishLdsPairs * 2);
    L.total = o;
    return L;
}

constexpr int kThinFull = 4, kThinHalf = 8;   // oracle THIN_FULL / THIN_HALF

// ---- (d3) manifolds + contact list, group ranges, min separation, wake, (f) prep, (g) colouring --------
// kPairsInLds: the scene's hull-pair list of this step (at most kFinishLdsPairs entries) and the per-pair scratch live in LDS --
// nearly every scene-step; longer lists are walked where they lie in global memory (same code, same results)
template <bool kPairsInLds, bool kFileLpt>
__device__ __forceinline__ void finish_scene(char* smem, const int s, const unsigned n_scenes, const slhip_settle_scene* __restrict__ scenes,
                                             slhip_body* bodies_all, const slhip_settle_params& prm, const WideBufs& W, const FinishLds& L, unsigned step)
{
    const int lane = threadIdx.x;
    WideHdr* H = W.hdr + s;
    WBody* wb = reinterpret_cast<WBody*>(smem + L.off_wb);
    Group* groups = reinterpret_cast<Group*>(smem + L.off_groups);
    HullPair* hp;
    unsigned short *hp_off, *hp_grp;
    if constexpr (kPairsInLds) {
        hp = reinterpret_cast<HullPair*>(smem + L.off_hp);
        hp_off = reinterpret_cast<unsigned short*>(smem + L.off_hp_off);
        hp_grp = reinterpret_cast<unsigned short*>(smem + L.off_hp_grp);
        const HullPair* g = W.hp + (size_t)s * W.p_cap;
        for (int k = lane; k < H->n_hp; k += 64) hp[k] = g[k];
    } else {
        hp = W.hp + (size_t)s * W.p_cap;
        hp_off = W.hp_off + (size_t)s * (W.p_cap + 1);
        hp_grp = W.hp_grp + (size_t)s * W.p_cap;
    }
    unsigned short* order = reinterpret_cast<unsigned short*>(smem + L.off_order);
    const slhip_settle_scene sc = scenes[s];
    slhip_body* bodies = bodies_all + sc.body_begin;
    const int nb = (int)(sc.body_end - sc.body_begin);
    unsigned long long* used = reinterpret_cast<unsigned long long*>(smem + L.off_misc);
    int* wake = reinterpret_cast<int*>(smem + L.off_misc + nb * 8);
    int* sep_key = reinterpret_cast<int*>(smem + L.off_misc + nb * 12);
    int* counters = reinterpret_cast<int*>(smem + L.off_misc + nb * 16);
    const int c_cap = W.c_cap, g_cap = W.g_cap;
    Contact* ac = W.ac + (size_t)s * c_cap;
    const int n_hp = H->n_hp, n_groups = H->n_groups, n_plane_groups = H->n_plane_groups;
    const int plane_offered = H->n_active_before_pairs;
    const int n_active_before_pairs = min(plane_offered, c_cap);
    int n_active = n_active_before_pairs;
    int* gcp = reinterpret_cast<int*>(smem + L.off_gcnt);      // contact pairs of the group
    int* gsum = gcp + g_cap;                                   // points its hull pairs offer (after thinning)
    int* gk0 = gsum + g_cap;                                   // its first hull pair
    unsigned short* cstart = order + g_cap;
    const MainResult* mrs = W.mr + (size_t)s * W.p_cap;
    const StagePt* stage = W.stage + (size_t)s * W.p_cap * 4;   // the points of every contact pair's manifold

    wave_copy_words(wb, W.wb + (size_t)s * W.nb_cap, nb * (int)sizeof(WBody), lane);
    for (int g = lane; g < n_groups; g += 64) { groups[g] = W.groups[(size_t)s * g_cap + g]; gcp[g] = 0; gsum[g] = 0; gk0[g] = 0; }
    for (int k = lane; k <= n_hp; k += 64) hp_off[k] = 0;
    for (int i = lane; i < nb; i += 64) { wake[i] = 0; sep_key[i] = 0x7f7fffff; }
    __syncthreads();

    // the pair group of every hull pair (the hull pairs of a body pair are contiguous), contact pairs per group
    {
        int gi = n_plane_groups;
        for (int base = 0; base < n_hp; base += 64) {
            const int k = base + lane;
            bool first = false;
            if (k < n_hp) first = k == 0 || hp_key(hp[k - 1]) != hp_key(hp[k]);
            const unsigned long long fm = __ballot(first);
            const int gk = gi + (int)__popcll(fm & ((2ull << lane) - 1ull)) - 1;
            if (k < n_hp) {
                hp_grp[k] = (unsigned short)gk;
                if (first) gk0[gk] = k;
                if (mrs[k].type != 0) atomicAdd(&gcp[gk], 1);
            }
            gi += (int)__popcll(fm);
        }
    }
    __syncthreads();

    // (d3) per hull pair: the manifold the narrowphase parked in the pair's stage slots (k_w_gjk_*: the kept one, refreshed;
    // k_w_manifold: the built one), thinned when the body pair touches through many hull pairs (oracle: all four points up to
    // THIN_FULL contact pairs, two up to THIN_HALF, one beyond)
    const PM* pm_prev = W.pm + ((size_t)((step - 1u) & 1u) * n_scenes + s) * W.p_cap;
    PM* pm_cur = W.pm + ((size_t)(step & 1u) * n_scenes + s) * W.p_cap;
    int offered_run = 0;
    for (int base = 0; base < n_hp; base += 64) {
        const int k = base + lane;
        int cnt = 0;
        if (k < n_hp) {
            const MainResult mm = mrs[k];
            if (mm.type != 0) {
                const HullPair e = hp[k];
                const int bi = hp_ba(e), bj = hp_bb(e);
                const int have = mm.seed.i1;
                float smin = kInf;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc)
                    if (cc < have) { const float sp = stage[4 * k + cc].sp; if (sp < smin) smin = sp; }
                int key = __float_as_int(smin);
                key = key >= 0 ? key : key ^ 0x7fffffff;
                atomicMin(&sep_key[bi], key);
                atomicMin(&sep_key[bj], key);
                const int ncp = gcp[hp_grp[k]];
                const int limit = ncp <= kThinFull ? 4 : ncp <= kThinHalf ? 2 : 1;
                cnt = min(have, limit);
            }
        }
        if (k < n_hp) {
            hp_off[k] = (unsigned short)cnt;
            if (cnt > 0) atomicAdd(&gsum[hp_grp[k]], cnt);
        }
        int total = cnt + (cnt >= 3 ? 1 : 0);              // (+ the centre row of a patch of three or four points)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
        offered_run += total;
    }
    __syncthreads();

    // Compound manifold reduction (slhip_settle_params.pair_contact_budget, oracle step_scene; not in the reference): a body pair
    // offering more points than the budget B keeps the hull pairs with the deepest points, ties in list order.  B >= 16 means such a
    // group is in the one-point-per-hull-pair regime of the thinning, so the choice is among hull pairs.  The B-th smallest key by
    // bisection over the key bits, then the keepers are marked in list order; the others stay filed as manifolds (kCulled).
    int B = (int)prm.pair_contact_budget;
    if (B > 0 && B < 16) B = 16;
    bool reduced = false;
    if (B > 0)
        for (int g0 = n_plane_groups; g0 < n_groups; g0 += 64) {
            const int gl = g0 + lane;
            unsigned long long over = __ballot(gl < n_groups && gsum[gl] > B);
            while (over) {
                const int g = g0 + __ffsll((long long)over) - 1;
                over &= over - 1;
                reduced = true;
                const int k0 = gk0[g], k1 = g + 1 < n_groups ? gk0[g + 1] : n_hp;
                auto ukey = [&](int k) -> unsigned {       // float order as unsigned order
                    int key = __float_as_int(stage[4 * k].sp);
                    key = key >= 0 ? key : key ^ 0x7fffffff;
                    return (unsigned)key ^ 0x80000000u;
                };
                unsigned T = 0u;
                for (int bit = 31; bit >= 0; --bit) {
                    const unsigned cand = T | (1u << bit);
                    int below = 0;
                    for (int kb = k0; kb < k1; kb += 64) {
                        const int k = kb + lane;
                        below += (int)__popcll(__ballot(k < k1 && hp_off[k] != 0 && ukey(k) < cand));
                    }
                    if (below <= B - 1) T = cand;
                }
                int less = 0;
                for (int kb = k0; kb < k1; kb += 64) {
                    const int k = kb + lane;
                    less += (int)__popcll(__ballot(k < k1 && hp_off[k] != 0 && ukey(k) < T));
                }
                int quota = B - less;                      // of the points AT the threshold, the first `quota` in list order stay
                for (int kb = k0; kb < k1; kb += 64) {
                    const int k = kb + lane;
                    const bool has = k < k1 && hp_off[k] != 0;
                    const unsigned uk = has ? ukey(k) : 0u;
                    const bool tie = has && uk == T;
                    const unsigned long long tm = __ballot(tie);
                    const int rank = (int)__popcll(tm & ((1ull << lane) - 1ull));
                    if (has && (uk > T || (tie && rank >= quota))) hp_off[k] = kCulled;
                    quota -= min(quota, (int)__popcll(tm));
                }
            }
        }
    int culled_run = 0;                                     // the culled points are no longer offered to the solver
    if (reduced) {
        for (int kb = 0; kb < n_hp; kb += 64) {
            const int k = kb + lane;
            culled_run += (int)__popcll(__ballot(k < n_hp && hp_off[k] == kCulled));
        }
        offered_run -= culled_run;
        __syncthreads();
    }

    // PhysX has no contact cap (scene.cpp:738-739): the solver takes every contact the step offers -- from LDS as far as the
    // scene's wave holds them, the rest from global memory.  What goes beyond the capacity the caller gave the list is dropped in list
    // order by the appends below, and counted.
    if (lane == 0) {
        const int offered = plane_offered + offered_run;
        unsigned* cp = W.caps + (size_t)kCapWords * s;
        if (offered > c_cap) atomicAdd(&cp[kCapContactDropSteps], 1u);
        if (H->hp_overflow) atomicAdd(&cp[kCapPairDropSteps], 1u);
        if (reduced) atomicAdd(&cp[kCapReducedSteps], 1u);
        if (H->g_overflow) atomicAdd(&cp[kCapGroupDropSteps], 1u);
        atomicMax(&cp[kCapMaxContacts], (unsigned)offered);
        atomicMax(&cp[kCapMaxPairs], (unsigned)H->hp_found);
    }

    // contacts appended in pair order from the parked points; the manifold is filed for the next step
    for (int base = 0; base < n_hp; base += 64) {
        const int k = base + lane;
        const bool culled = k < n_hp && hp_off[k] == kCulled;
        const int kept = k < n_hp && !culled ? (int)hp_off[k] : 0;
        const int lead = kept >= 3 ? 1 : 0;                // the patch's centre row, at its head in the list (oracle patch_centre)
        int total;
        const int off = n_active + wave_excl_scan(kept + lead, total);
        if (culled) {
            // out of the solver this step, still the pair's manifold: it is refreshed (not rebuilt) next step, without impulse
            const HullPair e = hp[k];
            const int bi = hp_ba(e), bj = hp_bb(e);
            const StagePt t = stage[4 * k];
            PM out;
            out.nb = mrs[k].type == 3 ? pm_prev[mrs[k].seed.n].nb : m3_tmul(wb[bj].R, mrs[k].n);
            out.pad[0] = out.pad[1] = out.pad[2] = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) { out.la[cc] = V(0, 0, 0); out.lb[cc] = V(0, 0, 0); }
            out.la[0] = m3_tmul(wb[bi].R, sub(t.qa, wb[bi].t));
            out.lb[0] = m3_tmul(wb[bj].R, sub(t.qb, wb[bj].t));
            out.count = 1; out.c_off = -1;
            pm_cur[k] = out;
        } else if (kept > 0) {
            const HullPair e = hp[k];
            const int bi = hp_ba(e), bj = hp_bb(e);
            const v3 n = mrs[k].n;
            const float rest = 2.0f * prm.rest_offset;
            const float er = 0.5f * (bodies[bi].restitution + bodies[bj].restitution);
            int written = 0;
            PM out;
            out.nb = mrs[k].type == 3 ? pm_prev[mrs[k].seed.n].nb : m3_tmul(wb[bj].R, n);   // the normal the manifold was built with
            out.pad[0] = out.pad[1] = out.pad[2] = 0.0f;
            v3 sra = V(0, 0, 0), srb = V(0, 0, 0);
            float ssp = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                out.la[cc] = V(0, 0, 0); out.lb[cc] = V(0, 0, 0);
                if (cc < kept) {
                    const StagePt t = stage[4 * k + cc];
                    if (lead) { sra = add(sra, sub(t.qa, wb[bi].x)); srb = add(srb, sub(t.qb, wb[bj].x)); ssp = ssp + t.sp; }
                    if (off + lead + cc < c_cap) {
                        fill_contact(&ac[off + lead + cc], bi, bj, wb[bi], &wb[bj], t.qa, t.qb, n, t.sp, rest, er, cc == 0 && !lead,
                                     kWarmStart * __int_as_float(t.imp));
                        out.la[cc] = m3_tmul(wb[bi].R, sub(t.qa, wb[bi].t));
                        out.lb[cc] = m3_tmul(wb[bj].R, sub(t.qb, wb[bj].t));
                        ++written;
                    }
                }
            }
            if (lead && off < c_cap) {
                // its impulse of the previous step: before the first point's in the step's impulse array, when that step filed the
                // pair's manifold with a centre row (with or without points behind it)
                float carried = 0.0f;
                if (mrs[k].seed.i0) {
                    const PM& pv = pm_prev[mrs[k].seed.n];
                    if (pv.c_off > 0 && pv.pad[0] != 0.0f) carried = kWarmStart * (W.lnout + (size_t)s * c_cap)[pv.c_off - 1];
                }
                fill_centre(&ac[off], bi, bj, kept, sra, srb, ssp, n, rest, er, carried);
                out.pad[0] = 1.0f;
            }
            out.count = written; out.c_off = min(off + lead, c_cap);   // (the first POINT's impulse) points beyond the capacity leave the manifold
            pm_cur[k] = out;
        } else if (k < n_hp && mrs[k].type != 0) {
            PM out;
            out.count = 0; out.c_off = 0; out.nb = V(0, 0, 0);
            out.pad[0] = out.pad[1] = out.pad[2] = 0.0f;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) { out.la[cc] = V(0, 0, 0); out.lb[cc] = V(0, 0, 0); }
            pm_cur[k] = out;
        }
        if (k < n_hp) hp_off[k] = (unsigned short)min(off, c_cap);   // from here on: the pair's first contact
        n_active = min(n_active + total, c_cap);
    }
    if (lane == 0) hp_off[n_hp] = (unsigned short)n_active;
    __syncthreads();
    // a pair group's contact range: from the offset of its first hull pair to the end of its last one
    for (int k = lane; k < n_hp; k += 64) {
        const unsigned key = hp_key(hp[k]);
        if (k == 0 || hp_key(hp[k - 1]) != key) groups[hp_grp[k]].begin = hp_off[k];
        if (k == n_hp - 1 || hp_key(hp[k + 1]) != key) groups[hp_grp[k]].end = hp_off[k + 1];
    }
    for (int i = lane; i < nb; i += 64) {
        int key = sep_key[i];
        key = key >= 0 ? key : key ^ 0x7fffffff;
        const float sv = __int_as_float(key);
        bodies[i].separation = sv > kInf ? kInf : sv;
    }
    __threadfence_block();
    __syncthreads();

    // wake sleeping bodies touched by a moving body (pair groups only)
    for (int g = n_plane_groups + lane; g < n_groups; g += 64) {
        const Group G = groups[g];
        bool touching = false;
        for (int c = G.begin; c < G.end; ++c)
            if (ac[c].err + 2.0f * prm.rest_offset < 2.0f * prm.contact_offset) touching = true;
        if (!touching) continue;
        for (int sd = 0; sd < 2; ++sd) {
            const int me = sd ? G.b : G.a, other = sd ? G.a : G.b;
            if ((bodies[me].flags & SLHIP_BODY_ASLEEP) && wb[other].dynamic) {
                const float en = 0.5f * dot(wb[other].v, wb[other].v);
                if (en > prm.sleep_threshold) wake[me] = 1;
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < nb; i += 64)
        if (wake[i]) {
            bodies[i].flags &= ~SLHIP_BODY_ASLEEP;
            bodies[i].wake_counter = prm.wake_time;
        }

    // (f) prep
    for (int c = lane; c < n_active; c += 64) prep_contact(&ac[c], wb, prm.bounce_threshold, 1.0f / prm.dt);
    // (g) greedy colouring, largest group first (oracle color_groups)
    for (int g0 = 0; g0 < n_groups; g0 += 64) {
        const int g = g0 + lane;
        if (g < n_groups) {
            const int sz = (int)groups[g].end - (int)groups[g].begin;
            int rank = 0;
            for (int h = 0; h < n_groups; ++h) {
                const int sh = (int)groups[h].end - (int)groups[h].begin;
                rank += (sh > sz || (sh == sz && h < g)) ? 1 : 0;
            }
            order[rank] = (unsigned short)g;
        }
    }
    __syncthreads();
    if (lane == 0) {
        for (int i = 0; i < nb; ++i) used[i] = 0ull;
        // the lowest of the colours 0..62 that neither body uses; a group whose bodies leave none free (a hub with more than 63
        // neighbours) gets a colour of its own from 63 on
        int ncol = 0, extra = 63;
        for (int q = 0; q < n_groups; ++q) {
            const int g = order[q];
            const int a = groups[g].a, b = groups[g].b == kNoBody ? -1 : (int)groups[g].b;
            unsigned long long m = used[a];
            if (b >= 0) m |= used[b];
            int c = 0;
            while (c < 63 && ((m >> c) & 1ull)) ++c;
            if (c == 63) c = extra++;
            else {
                used[a] |= 1ull << c;
                if (b >= 0) used[b] |= 1ull << c;
            }
            groups[g].color = (unsigned short)c;
            if (c + 1 > ncol) ncol = c + 1;
        }
        counters[1] = ncol;
    }
    __syncthreads();
    const int ncol = counters[1];
    {
        int base = 0;
        for (int col = 0; col < ncol; ++col) {
            if (lane == 0) cstart[col] = (unsigned short)base;
            for (int g0 = 0; g0 < n_groups; g0 += 64) {
                const int g = g0 + lane;
                const bool p = g < n_groups && groups[g].color == col;
                const int slot = compact_slot(p, base);
                if (p) order[slot] = (unsigned short)g;
                base += __popcll(__ballot(p));
            }
        }
        if (lane == 0) cstart[ncol] = (unsigned short)base;
    }
    __syncthreads();
    // Stabilisation (PxSceneFlag::eENABLE_STABILIZATION, oracle step_scene): per body the body pairs it touches through this step's
    // contacts, and whether its island rests on something that does not move (the table, a static or a sleeping body) -- the flag
    // spreads over the groups of two dynamic bodies until nothing changes.  Handed to the solver in the working body's `dynamic`
    // word: bit 0 dynamic, bit 1 rests on something static, bits 8.. the pairs (the solver reads the word as a boolean elsewhere).
    if (prm.stabilization_threshold > 0.0f) {
        int* st = wake;                                    // (the wake flags are spent)
        for (int i = lane; i < nb; i += 64) st[i] = 0;
        __syncthreads();
        for (int g = lane; g < n_groups; g += 64) {
            const Group G = groups[g];
            if (G.end <= G.begin) continue;
            const int a = G.a, b = G.b == kNoBody ? -1 : (int)G.b;
            atomicAdd(&st[a], 0x100);
            if (b >= 0) atomicAdd(&st[b], 0x100);
            if (b < 0 || !wb[b].dynamic) atomicOr(&st[a], 2);
            if (b >= 0 && !wb[a].dynamic) atomicOr(&st[b], 2);
        }
        __syncthreads();
        for (;;) {
            bool changed = false;
            for (int g = lane; g < n_groups; g += 64) {
                const Group G = groups[g];
                if (G.end <= G.begin || G.b == kNoBody) continue;
                const int a = G.a, b = (int)G.b;
                if (!wb[a].dynamic || !wb[b].dynamic) continue;
                const int ta = st[a] & 2, tb = st[b] & 2;
                if (ta == tb) continue;
                atomicOr(&st[a], 2);
                atomicOr(&st[b], 2);
                changed = true;
            }
            __syncthreads();
            if (__ballot(changed) == 0ull) break;
        }
        WBody* gw = W.wb + (size_t)s * W.nb_cap;
        for (int i = lane; i < nb; i += 64)
            if (wb[i].dynamic) gw[i].dynamic = 1 | st[i];
    }
    // hand over to the solver: groups (ranges + colours), the colour-ordered list, the colours' first slots
    for (int g = lane; g < n_groups; g += 64) W.groups[(size_t)s * g_cap + g] = groups[g];
    unsigned short* og = W.order + (size_t)s * W.o_stride;
    for (int k = lane; k < n_groups; k += 64) og[k] = order[k];
    for (int k = lane; k <= ncol; k += 64) og[g_cap + k] = cstart[k];
    if (lane == 0) { H->n_active = n_active; H->ncol = ncol; W.caps[(size_t)kCapWords * s + kCapContactSum] += (unsigned)n_active; }
    // The solver's cost for this scene = what a lane pair walks in sequence per sweep: per colour the largest group.  The
    // scene joins its cost bucket; k_w_solve hands its blocks out costliest first, so the long scenes (a p99 chain is five
    // times the mean) start at the beginning of the launch instead of anywhere -- including its last moments.
    int chain = 0;
    for (int col = 0; kFileLpt && col < ncol; ++col) {
        int mx = 0;
        for (int g = lane; g < n_groups; g += 64)
            if (groups[g].color == col) mx = max(mx, (int)groups[g].end - (int)groups[g].begin);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        chain += mx;
    }
    if (lane == 0) {
        // The LDS the scene's solve wants this step (solve_need): working bodies, groups, colour lists, every contact.  Scenes that
        // fit a quarter of a solver wave's LDS share a wave by four, those that fit a half by two (lane groups of 16 / 32: a wave64
        // instruction costs the same whatever its lane count, and most scene-steps are light), the others take a wave of their own
        // and keep as many contacts in LDS as fit, the rest being swept from global memory.
        const int need = solve_need(nb, n_groups, ncol, n_active);
        int cls = need <= W.solve_lds / 4 ? 2 : need <= W.solve_lds / 2 ? 1 : 0;
        if (cls > W.solve_max_class) cls = W.solve_max_class;
        H->lds_need = need; H->lds_class = cls;
        if (need > W.solve_lds) atomicAdd(&W.caps[(size_t)kCapWords * s + kCapSpillSteps], 1u);      // (a wave of its own, and still not everything fits)
        // 32 cost classes x 8 shards (scene & 7): while everything still falls, all scenes are in class 0 -- 16384 atomics on one
        // address queue up for ~10 ns each, on eight addresses they do not
        if (kFileLpt) {
            const int bucket = min(chain >> 3, 31) * 8 + (s & 7);
            // counters are stored shard-major: the eight shards of a class lie 128 bytes apart, i.e. in eight cache lines
            const unsigned r = atomicAdd(&W.lpt_count[cls * 256 + (bucket & 7) * 32 + (bucket >> 3)], 1u);
            W.lpt_table[((size_t)cls * 256 + bucket) * ((n_scenes + 7u) / 8u) + r] = (unsigned short)s;
            atomicAdd(&W.lpt_count[3 * 256 + cls * 8 + (s & 7)], 1u);
        }
    }
}

// the finish of one scene-step: the pair cache's table of the previous step emptied, then finish_scene
template <bool kFileLpt>
__device__ __forceinline__ void finish_step(char* smem, const int s, const unsigned n_scenes, const slhip_settle_scene* __restrict__ scenes,
                                            slhip_body* bodies_all, const slhip_settle_params& prm, const WideBufs& W, const FinishLds& L,
                                            const PairCache& pc, unsigned step)
{
    const int lane = threadIdx.x;
    WideHdr* H = W.hdr + s;
    if (H->status != 0) return;
    if (pc.hashed) {
        // the hashed pair cache: this step's GJK passes were the last readers of the table the previous step filled -- emptied now,
        // it is the table the next step files its pairs in
        const unsigned half = pc.stride >> 1;
        int4* z = pc.base + (size_t)s * pc.stride + (size_t)((step - 1u) & 1u) * half;
        for (unsigned k = lane; k < half; k += 64) z[k] = make_int4(0, 0, 0, 0);
    }
    if (H->n_hp <= kFinishLdsPairs) finish_scene<true, kFileLpt>(smem, s, n_scenes, scenes, bodies_all, prm, W, L, step);
    else finish_scene<false, kFileLpt>(smem, s, n_scenes, scenes, bodies_all, prm, W, L, step);
}

__global__ __launch_bounds__(64) void k_w_finish(const slhip_settle_scene* __restrict__ scenes, slhip_body* bodies_all,
                                                slhip_settle_params prm, WideBufs W, FinishLds L, PairCache pc, unsigned step)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (blockIdx.x == 0 && threadIdx.x < 16) W.work_count[threadIdx.x] = 0u;   // the work lists of this step are spent
    finish_step<true>(smem, (int)blockIdx.x, gridDim.x, scenes, bodies_all, prm, W, L, pc, step);
}

// The least LDS a solver wave must have: a scene of the batch's largest shape (nb_cap bodies, g_cap groups and as many colours)
// with a few contacts resident -- the rest of such a scene's contacts is swept from global memory.
__host__ __device__ inline int solve_min_lds(int nb_cap, int g_cap) { return solve_need(nb_cap, g_cap, g_cap + 64, 16); }

// the scenes of ranks `rank0 .. rank0 + 3` of wave class `cls` in descending cost order (cost classes of k_w_finish, arrival
// order within a class); -1: none.  All 64 lanes of the wave take part.  The 256 class counts are fetched with four loads in
// flight and scanned once for all four ranks (one memory round trip for the counts, one for the table entries).
__device__ __forceinline__ void lpt_scenes(const WideBufs& W, int cls, unsigned rank0, unsigned n_scenes, int lane, int (&out)[4])
{
    constexpr int kN = 4;
    const unsigned per = (n_scenes + 7u) / 8u;
    const unsigned* count = W.lpt_count + cls * 256;
    const unsigned short* table = W.lpt_table + (size_t)cls * 256 * per;
    unsigned cnt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 255 - (q * 64 + lane);
        cnt[q] = count[(c & 7) * 32 + (c >> 3)];
    }
    unsigned run = 0u;
    size_t slot[kN];
    bool have[kN];
#pragma unroll
    for (int r = 0; r < kN; ++r) { have[r] = false; slot[r] = 0; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = 255 - (q * 64 + lane);
        int total;
        const unsigned ex = run + (unsigned)wave_excl_scan((int)cnt[q], total);
#pragma unroll
        for (int r = 0; r < kN; ++r) {
            const unsigned rank = rank0 + (unsigned)r;
            const unsigned long long m = __ballot(rank >= ex && rank < ex + cnt[q]);
            if (m != 0ull && !have[r]) {
                const int src = __ffsll((long long)m) - 1;
                const int bucket = __shfl(c, src, 64);
                const unsigned first = (unsigned)__shfl((int)ex, src, 64);
                slot[r] = (size_t)bucket * per + (rank - first);
                have[r] = true;
            }
        }
        run += (unsigned)total;
    }
#pragma unroll
    for (int r = 0; r < kN; ++r) out[r] = have[r] ? (int)table[slot[r]] : -1;
}

// dword copies by the `n_lanes` lanes of a sub-wave (lane index `hl`)
__device__ __forceinline__ void sub_copy_words(void* dst, const void* src, int bytes, int hl, int n_lanes) { lanes_copy(dst, src, bytes, hl, n_lanes); }

// ---- (h) position iterations, (i) integrate, (j) velocity iterations, (k) store + sleep, frame end: redrop
// ONE launch, waves of one, two or four scenes (the wave classes of k_w_finish): the sweeps are bound by VALU issue with a
// handful of the 64 lanes active, and a wave64 instruction costs the same whatever its lane count -- light scenes (most
// scene-steps) share a wave by four, 16 lanes each, their state packed into the wave's LDS by what they need; a heavy scene has
// the wave, and its LDS, to itself.  The blocks take the classes heaviest first and, within a class, the scenes in descending
// cost order, i.e. neighbours in the cost classes side by side: their sweeps walk chains of similar length, so a wave runs about
// as long as ONE of its scenes would.  Every scene is solved exactly as before -- by its own lanes, same bits.
// The solve of the wave's scenes: lane `lane` works for scene `s` (-1: none) of a wave of class `cls` holding `spw` scenes.
__device__ __forceinline__ void solve_wave(char* smem_all, const int cls, const int spw, int s, const slhip_settle_scene* __restrict__ scenes,
                                           slhip_body* bodies_all, const slhip_settle_params& prm, const WideBufs& W, DriveAcc* drive_all,
                                           const int end_of_frame);

__global__ __launch_bounds__(64) void k_w_solve(const slhip_settle_scene* __restrict__ scenes, slhip_body* bodies_all,
                                               slhip_settle_params prm, WideBufs W, DriveAcc* drive_all,
                                               int end_of_frame, unsigned n_scenes)
{
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    const int lane = threadIdx.x;
    // which wave of which class is this block?
    int cls, spw;
    unsigned rank0;
    {
        unsigned part = lane < 24 ? W.lpt_count[3 * 256 + lane] : 0u;      // the classes' totals: eight shards each
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) part += __shfl_xor(part, o, 64);
        const unsigned t0 = (unsigned)__shfl((int)part, 0, 64), t1 = (unsigned)__shfl((int)part, 8, 64), t2 = (unsigned)__shfl((int)part, 16, 64);
        const unsigned w0 = t0, w1 = (t1 + 1u) / 2u, w2 = (t2 + 3u) / 4u, b = blockIdx.x;
        if (b < w0) { cls = 0; spw = 1; rank0 = b; }
        else if (b < w0 + w1) { cls = 1; spw = 2; rank0 = (b - w0) * 2u; }
        else if (b < w0 + w1 + w2) { cls = 2; spw = 4; rank0 = (b - w0 - w1) * 4u; }
        else return;
    }
    const int kLanes = 64 / spw;                       // lanes per scene
    const int slot = lane / kLanes;
    int s = -1;
    {
        int ranked[4];
        lpt_scenes(W, cls, rank0, n_scenes, lane, ranked);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q == slot) s = ranked[q];
    }
    solve_wave(smem_all, cls, spw, s, scenes, bodies_all, prm, W, drive_all, end_of_frame);
}

__device__ __forceinline__ void solve_wave(char* smem_all, const int cls, const int spw, int s, const slhip_settle_scene* __restrict__ scenes,
                                           slhip_body* bodies_all, const slhip_settle_params& prm, const WideBufs& W, DriveAcc* drive_all,
                                           const int end_of_frame)
{
    const int lane = threadIdx.x;
    const int kLanes = 64 / spw;                       // lanes per scene
    const int slot = lane / kLanes, hl = lane % kLanes;
    bool on = s >= 0;                                  // the class's last wave may hold fewer scenes than slots
    const WideHdr* H = W.hdr + (on ? s : 0);
    if (on && H->status != 0) on = false;
    const slhip_settle_scene sc = scenes[on ? s : 0];
    slhip_body* bodies = bodies_all + sc.body_begin;
    const int nb = on ? (int)(sc.body_end - sc.body_begin) : 0;
    DriveAcc* drv = drive_all + (size_t)(on ? s : 0) * W.nb_cap;
    const int n_groups = on ? H->n_groups : 0, ncol = on ? H->ncol : 0;
    const int n_active = on ? H->n_active : 0;
    // the scene's share of the wave's LDS: packed behind the scenes of the slots before it
    auto al = [](int b) { return (b + 15) & ~15; };
    const int need = on ? H->lds_need : 0;
    int base = 0;
    for (int q = 0; q < 3; ++q) {
        const int nq = __shfl(need, q * kLanes < 64 ? q * kLanes : 0, 64);
        if (q < slot && q < spw) base += nq;
    }
    char* smem = smem_all + base;
    const int off_groups = al(nb * (int)sizeof(SBody)), off_order = off_groups + al(n_groups * (int)sizeof(Group));
    const int off_contacts = off_order + al((n_groups + ncol + 2) * 2);
    // the solver's part of the working bodies in LDS (SBody = the tail of WBody), their poses where k_w_begin left them in the scratch
    SBody* wb = reinterpret_cast<SBody*>(smem);
    WBody* gw = W.wb + (size_t)(on ? s : 0) * W.nb_cap;
    Group* groups = reinterpret_cast<Group*>(smem + off_groups);
    unsigned short* order = reinterpret_cast<unsigned short*>(smem + off_order);
    unsigned short* cstart = order + n_groups;
    // The scene's contacts are pulled into LDS once (one coalesced read): every sweep walks them in dependent order, and an L2
    // round trip per contact and sweep costs several times the arithmetic.  A scene of the one- and two-scene... of the shared
    // classes has ALL its contacts there (that is what its class says); a scene with a wave of its own keeps as many as the
    // wave's LDS holds and sweeps the rest in place in its list in global memory, the next contact fetched while the current
    // row runs: the list has no cap but the capacity the caller gave it.
    ContactList ac;
    ac.lds = reinterpret_cast<Contact*>(smem + off_contacts);
    ac.glb = W.ac + (size_t)(on ? s : 0) * W.c_cap;
    ac.n_lds = cls == 0 ? min(n_active, max(0, (W.solve_lds - off_contacts) / (int)sizeof(Contact))) : n_active;
    const float dt = prm.dt;

    // what the later phases need of the lane's own first body (i = hl) is fetched now, with the copies below in flight: fetched where
    // it is used, every item is a memory round trip of its own on the wave's critical path.  (Bodies beyond the first kLanes of a
    // scene -- scenes of more than 64 bodies at one scene per wave -- read theirs where they need it.)
    float bc_lim = 0.0f, bc_wake = 0.0f, bc_com[3] = {0.0f, 0.0f, 0.0f}, bc_L[9], bc_st0 = 0.0f, bc_st1 = 0.0f;
    unsigned bc_drive = 0u, bc_flags = 0u;
#pragma unroll
    for (int c = 0; c < 9; ++c) bc_L[c] = 0.0f;
    if (hl < nb) {
        const slhip_body& B = bodies[hl];
        bc_lim = B.max_lin_vel; bc_wake = B.wake_counter; bc_drive = B.drive_flags;
        bc_st0 = B.stab[0]; bc_st1 = B.stab[1]; bc_flags = B.flags;
#pragma unroll
        for (int c = 0; c < 3; ++c) bc_com[c] = B.com[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) bc_L[3 * r + c] = B.inv_inertia[4 * r + c];
    }
    if (on) {
        {
            const unsigned* src = reinterpret_cast<const unsigned*>(gw);
            unsigned* dst = reinterpret_cast<unsigned*>(wb);
            for (int q = hl; q < nb * kSBodyWords; q += kLanes) {
                const int bi = q / kSBodyWords, wi = q - bi * kSBodyWords;
                dst[q] = src[bi * kWBodyWords + (kWBodyWords - kSBodyWords) + wi];
            }
        }
        sub_copy_words(ac.lds, ac.glb, ac.n_lds * (int)sizeof(Contact), hl, kLanes);
        for (int g = hl; g < n_groups; g += kLanes) groups[g] = W.groups[(size_t)s * W.g_cap + g];
        const unsigned short* og = W.order + (size_t)s * W.o_stride;
        for (int k = hl; k < n_groups; k += kLanes) order[k] = og[k];
        for (int k = hl; k <= ncol; k += kLanes) cstart[k] = og[W.g_cap + k];
    }
    __syncthreads();
    int ncol_max = ncol;                               // the wave's colour loop: as long as its longest scene needs
    for (int o = kLanes; o < 64; o <<= 1) ncol_max = max(ncol_max, __shfl_xor(ncol_max, o, 64));

    const float inv_dt = 1.0f / prm.dt;
    // warm start: the carried normal impulses (fill_contact) are applied to the bodies in the sweeps' order before the first sweep
    for (int col = 0; col < ncol_max; ++col) {
        if (col < ncol) {
            const int ce = cstart[col + 1];
            for (int k = cstart[col] + (hl >> 1); k < ce; k += kLanes / 2) {
                const Group G = groups[order[k]];
                warm_group(ac, G.begin, G.end, G.a, G.b == kNoBody ? -1 : (int)G.b, hl & 1, wb);
            }
        }
        __syncthreads();
    }
    for (unsigned it = 0; it < prm.pos_iters; ++it) {
        for (int col = 0; col < ncol_max; ++col) {
            if (col < ncol) {
                const int ce = cstart[col + 1];
                for (int k = cstart[col] + (hl >> 1); k < ce; k += kLanes / 2) {   // a lane pair per group
                    const Group G = groups[order[k]];
                    solve_group(ac, G.begin, G.end, G.a, G.b == kNoBody ? -1 : (int)G.b, hl & 1, wb, inv_dt, true, prm.plane_mu_s, prm.plane_mu_d);
                }
            }
            __syncthreads();
        }
        for (int i = hl; i < nb; i += kLanes) {
            const unsigned df = i == hl ? bc_drive : bodies[i].drive_flags;
            if (df & 1u) drive_body(bodies[i], gw[i], wb[i], drv[i], prm, true);
        }
        __syncthreads();
    }
    // (i) integrate poses
    for (int i = hl; i < nb; i += kLanes) {
        if (!wb[i].dynamic) continue;
        const float lim = i == hl ? bc_lim : bodies[i].max_lin_vel;
        const float vv = dot(wb[i].v, wb[i].v);
        if (lim > 0.0f && vv > lim * lim) wb[i].v = scale(wb[i].v, lim / sqrtf(vv));
        const float ww = dot(wb[i].w, wb[i].w);
        const float wl = prm.max_angular_velocity;
        if (ww > wl * wl) wb[i].w = scale(wb[i].w, wl / sqrtf(ww));
        // the velocities that move the body this step: kept for the stabilisation's frame energy in the scratch body's rotation
        // matrix, which nothing reads until (k) rebuilds it from the quaternion
        WBody& g = gw[i];
        g.R.m[0] = wb[i].v.x; g.R.m[1] = wb[i].v.y; g.R.m[2] = wb[i].v.z;
        g.R.m[3] = wb[i].w.x; g.R.m[4] = wb[i].w.y; g.R.m[5] = wb[i].w.z;
        const quat q0 = g.q;
        g.x = madd(g.x, wb[i].v, dt);
        quat wq; wq.x = wb[i].w.x; wq.y = wb[i].w.y; wq.z = wb[i].w.z; wq.w = 0.0f;
        const quat dq = quat_mul(wq, q0);
        quat q;
        q.x = fmaf(0.5f * dt, dq.x, q0.x); q.y = fmaf(0.5f * dt, dq.y, q0.y);
        q.z = fmaf(0.5f * dt, dq.z, q0.z); q.w = fmaf(0.5f * dt, dq.w, q0.w);
        g.q = quat_normalize(q);
    }
    __syncthreads();
    for (unsigned it = 0; it < prm.vel_iters; ++it) {
        for (int col = 0; col < ncol_max; ++col) {
            if (col < ncol) {
                const int ce = cstart[col + 1];
                for (int k = cstart[col] + (hl >> 1); k < ce; k += kLanes / 2) {
                    const Group G = groups[order[k]];
                    solve_group(ac, G.begin, G.end, G.a, G.b == kNoBody ? -1 : (int)G.b, hl & 1, wb, inv_dt, false, prm.plane_mu_s, prm.plane_mu_d);
                }
            }
            __syncthreads();
        }
        for (int i = hl; i < nb; i += kLanes) {
            const unsigned df = i == hl ? bc_drive : bodies[i].drive_flags;
            if (df & 1u) drive_body(bodies[i], gw[i], wb[i], drv[i], prm, false);
        }
        __syncthreads();
    }
    // the impulses the manifolds carry into the next step
    if (on) {
        float* lo = W.lnout + (size_t)s * W.c_cap;
        for (int c = hl; c < n_active; c += kLanes) lo[c] = ac.ln(c);
    }
    // (k) store + sleep bookkeeping
    for (int i = hl; i < nb; i += kLanes) {
        if (!wb[i].dynamic) continue;
        const bool mine0 = i == hl;
        float com[3], Lm[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) com[c] = mine0 ? bc_com[c] : bodies[i].com[c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Lm[3 * r + c] = mine0 ? bc_L[3 * r + c] : bodies[i].inv_inertia[4 * r + c];
        const unsigned df = mine0 ? bc_drive : bodies[i].drive_flags;
        const float wk = mine0 ? bc_wake : bodies[i].wake_counter;
        WBody& g = gw[i];
        const v3 mv = V(g.R.m[0], g.R.m[1], g.R.m[2]), mw = V(g.R.m[3], g.R.m[4], g.R.m[5]);
        m3 R;
        quat_to_m3(g.q, R);
        const v3 t = sub(g.x, m3_mul(R, V(com[0], com[1], com[2])));
        // stabilisation (oracle step_scene (k); PhysX Dy::updateWakeCounter [ext])
        bool frozen = false;
        if (prm.stabilization_threshold > 0.0f) {
            const float fen = kinetic_energy(Lm, R, mv, mw, wb[i].inv_mass);
            const int word = wb[i].dynamic;
            const bool touch = (word & 2) != 0;
            const int ni = min(word >> 8, SLHIP_STAB_MAX_INTERACTIONS);
            const float thresh = touch ? (float)ni * prm.stabilization_threshold : 0.0f;
            float fc = (mine0 ? bc_st0 : bodies[i].stab[0]) + dt;
            float as = (1.0f - (mine0 ? bc_st1 : bodies[i].stab[1])) + dt;
            if (as > 1.0f) as = 1.0f;
            bool settled = true;
            if (fen >= thresh) { settled = false; fc = 0.0f; }
            if (!touch) { as = 1.0f; settled = false; }
            if (settled) {
                const float d = 1.0f - SLHIP_STAB_DAMPING * dt;
                wb[i].v = scale(wb[i].v, d);
                wb[i].w = scale(wb[i].w, d);
                as = as * 0.75f + 0.25f * SLHIP_STAB_GRAVITY;
                if (fc >= SLHIP_STAB_FREEZE_INTERVAL && fen < prm.stabilization_threshold * SLHIP_STAB_FREEZE_TOLERANCE) frozen = true;
            }
            bodies[i].stab[0] = fc;
            bodies[i].stab[1] = 1.0f - as;
        }
        unsigned fl = mine0 ? bc_flags : bodies[i].flags;
        fl = frozen ? (fl | SLHIP_BODY_FROZEN) : (fl & ~SLHIP_BODY_FROZEN);
        const float en = kinetic_energy(Lm, R, wb[i].v, wb[i].w, wb[i].inv_mass);
        if (en >= prm.sleep_threshold || (df & 1u)) bodies[i].wake_counter = prm.wake_time;
        else {
            const float wc = wk - dt;
            bodies[i].wake_counter = wc;
            if (wc <= 0.0f) {
                fl |= SLHIP_BODY_ASLEEP;
                wb[i].v = V(0, 0, 0);
                wb[i].w = V(0, 0, 0);
            }
        }
        bodies[i].flags = fl;
        if (!frozen) store_pose(bodies[i], R, t);           // (frozen: held in place, the step's pose change is taken back)
        store_velocities(bodies[i], wb[i].v, wb[i].w);
    }
    if (end_of_frame && prm.tabletop) {
        // redrop heuristic of simulateTableTopScene (scene.cpp:742-755).  Whether a body is dropped again depends on its own
        // record only (height, separation, stuck counter): every lane decides for its bodies; the drops themselves -- rare, and
        // each one looks at the poses the earlier ones left -- follow in body order
        __threadfence_block();
        __syncthreads();
        int nb_max = nb;                               // the wave's body loop: as long as its largest scene needs
        for (int o = kLanes; o < 64; o <<= 1) nb_max = max(nb_max, __shfl_xor(nb_max, o, 64));
        for (int i0 = 0; i0 < nb_max; i0 += kLanes) {
            const int i = i0 + hl;
            bool d = false;
            if (i < nb && !(bodies[i].flags & SLHIP_BODY_STATIC)) {
                if (bodies[i].pose[11] < prm.redrop_z) d = true;
                else if (bodies[i].separation < prm.stuck_separation) {
                    const int sc_new = bodies[i].stuck_counter + 1;
                    bodies[i].stuck_counter = sc_new;
                    d = sc_new > prm.stuck_frames;
                } else if (bodies[i].stuck_counter > 0) bodies[i].stuck_counter--;
            }
            const unsigned long long drop = __ballot(d);
            if (drop != 0ull) {
                // (the lanes that follow in this and the next rounds still decide on their own records: a redrop rewrites the
                // dropped body's pose and every body's sleep state, neither of which the decisions read -- except the dropped
                // body's own stuck counter, reset by the drop after its decision was taken, as in the oracle's loop)
                __threadfence_block();
                __syncthreads();
                if (on && hl == 0) {
                    unsigned long long m = (drop >> (slot * kLanes)) & (kLanes == 64 ? ~0ull : ((1ull << kLanes) - 1ull));
                    while (m != 0ull) {
                        const int b = __ffsll((long long)m) - 1;
                        m &= m - 1ull;
                        redrop(bodies, nb, i0 + b, prm);
                    }
                }
                __threadfence_block();
                __syncthreads();
            }
        }
    }
}

// ---- the same step, one scene per wave, every step of the call in ONE launch --------------------------------------------------
// Scenes are independent (the reference's advance one PxScene each, src/job_queue.cpp:95-144): a wave takes a scene through all
// the steps of the call -- begin, the GJK runs of its own candidate pairs (64 at a time), the manifolds of its own contact pairs
// (eight at a time), finish, solve -- with nothing but workgroup barriers between the phases, then takes the next scene.  No launch
// boundary ends with the batch's slowest scene, no work list is shared, no wave classes: the phases are the functions of the
// lockstep kernels (begin_scene, gjk_work_item, manifold_items, finish_step, solve_wave), every pair and every scene computed by
// the same code on the same inputs -- the same bits (tests/test_gpu_settle.py runs both forms).  What it gives up: the lockstep
// form fills GJK / manifold waves with pairs of MANY scenes and packs light scenes four to a solver wave; this form runs a scene's
// phases one after the other on ONE wave.  It is the form for small batches (a handful of scenes: 2 400 dependent launches of
// ~25 us become one) -- slhip_settle picks by batch size (SLHIP_SETTLE_PERSISTENT=0/1 overrides).
// (one wave per SIMD: 256 VGPRs + 132 AGPRs, no scratch; asked for two the kernel spills 152 registers and is no faster at 2 048 scenes)
#ifndef SLHIP_PERSISTENT_WAVES
#define SLHIP_PERSISTENT_WAVES 1
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SLHIP_PERSISTENT_WAVES))) void k_w_persistent(const slhip_settle_scene* __restrict__ scenes, slhip_body* bodies_all,
                                                    const slhip_hull* __restrict__ hulls, const float* __restrict__ hull_verts,
                                                    slhip_settle_params prm, WideBufs W, BeginLds BL, FinishLds FL, PairCache pc,
                                                    DriveAcc* drive_all, unsigned list_stride, unsigned n_scenes)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float s_uwh[8][kFmStrip];
    const unsigned lane = threadIdx.x;
    for (unsigned s = blockIdx.x; s < n_scenes; s += gridDim.x) {
        if (W.hdr[s].status != 0) continue;                       // refused by the prologue: untouched, as in the lockstep form
        unsigned* mine = W.work + 4 * (size_t)list_stride + (size_t)s * W.p_cap;      // the scene's contact pairs to build, its own slice of list 2
        unsigned step = prm.resume;
#ifdef SLHIP_PERSISTENT_PROFILE
        long long tph[5] = {0, 0, 0, 0, 0}, tq = wall_clock64();
#define SLHIP_PH(i) { const long long t_ = wall_clock64(); tph[i] += t_ - tq; tq = t_; }
#else
#define SLHIP_PH(i)
#endif
        for (unsigned f = 0; f < prm.frames; ++f)
            for (unsigned sub = 0; sub < prm.substeps; ++sub, ++step) {
                begin_scene<false>(smem, (int)s, n_scenes, scenes, bodies_all, hulls, hull_verts, prm, W, BL, drive_all, step + 1u);
                __threadfence_block();
                __syncthreads();
                SLHIP_PH(0)
                const unsigned n_hp = (unsigned)W.hdr[s].n_hp;
                unsigned n_build = 0u;
                for (unsigned k0 = 0; k0 < n_hp; k0 += 64u) {
                    const unsigned k = k0 + lane;
                    const unsigned e = (s << W.pair_bits) | k;
                    bool unfinished = false;
                    int type = 0;
                    if (k < n_hp) type = gjk_work_item(e, hull_verts, prm, W, pc, kGjkMaxIter, step + 1u, n_scenes, unfinished);
                    const bool build = type == 1;
                    const unsigned long long m = __ballot(build);
                    if (build) mine[n_build + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = e;
                    n_build += (unsigned)__popcll(m);
                }
                __threadfence_block();
                __syncthreads();
                SLHIP_PH(1)
                manifold_items(hull_verts, prm, W, mine, n_build, 0u, 8u, s_uwh);
                __threadfence_block();
                __syncthreads();
                SLHIP_PH(2)
                finish_step<false>(smem, (int)s, n_scenes, scenes, bodies_all, prm, W, FL, pc, step + 1u);
                __threadfence_block();
                __syncthreads();
                SLHIP_PH(3)
                solve_wave(smem, 0, 1, (int)s, scenes, bodies_all, prm, W, drive_all, sub + 1u == prm.substeps ? 1 : 0);
                __threadfence_block();
                __syncthreads();
                SLHIP_PH(4)
            }
#ifdef SLHIP_PERSISTENT_PROFILE
        if (lane == 0 && s < 4u)
            printf("scene %u: begin %.1f  gjk %.1f  manifold %.1f  finish %.1f  solve %.1f ms (100 MHz clock)\n", s, tph[0] * 1e-5, tph[1] * 1e-5,
                   tph[2] * 1e-5, tph[3] * 1e-5, tph[4] * 1e-5);
#endif
#undef SLHIP_PH
    }
}
