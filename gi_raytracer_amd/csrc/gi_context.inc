// gi_context.inc -- gi_ctx and the parts it is made of.  Host code only; included by gi_kernels.hip behind the kernels and before everything that
// uses the context.  A part owns its buffers, and the functions that maintain them are its members or stand right below gi_ctx:
//
//   SceneStore    the device tables of the uploaded scene (upload)
//   PhotonStore   the photon map and the tables derived from it (install_photon_map, clear_photon_map, build_photon_*)
//   Tuning        every value taken from the environment when the context is made (from_env), and the two limits the setters change
//   StageClock    per-stage device times of the last streaming frame (begin, end, read)
//   StreamState   workspaces of the stream passes and the rounds (stream_alloc)
//   AuxPass       timer and LDS answer of an auxiliary pass: features, occlusion, baked light, denoiser, upsampler, bake, lightmap, reflection probe,
//                 probe visibility
// Behind gi_ctx, what the entries of every .inc file share: fail, pass_ms (gi_last_*_ms) and Entry (a host-pointer call's device side).
#include "gi_scratch.h"   // DevBuf, EventTimer, finish_to_host

struct gi_ctx;

namespace {

int fail(gi_ctx* c, int code, const std::string& msg);
#define HIP_TRY(c, expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess) return fail((c), GI_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// pinned host memory that frees itself: the mirror of a few device words a pass reads back
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t count)               // once: kept for the context's life
    {
        if (p) return hipSuccess;
        const hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------ the scene
struct SceneStore {
    bool have_scene = false;
    DevBuf<TNode> d_tnodes;
    DevBuf<WNode> d_wnodes;
    DevBuf<int32_t> d_wleaf_id;
    DevBuf<float> d_cboxes;               // content boxes of the wide records' children
    DevBuf<uint32_t> d_cuse;
    DevBuf<TexD> d_texs;
    DevBuf<TriUV> d_tri_uv;
    DevBuf<unsigned char> d_tex_pixels;
    DevBuf<double> d_tex_lut;
    DevBuf<int32_t> d_refs;
    DevBuf<LeafTri> d_leaf_tris;
    DevBuf<double> d_leaf_boxes;          // every leaf reference's own box (gi_walk.h: entity_survivors)
    DevBuf<double> d_trace_boxes;         // the closest-hit walk's boxes (gi_walk.h: trace_wide_step)
    DevBuf<float> d_tcboxes;              // and the content boxes made of them
    DevBuf<uint32_t> d_tcuse;
    WalkCuts cuts;                        // of the scene last uploaded: what it allows the walks' short cuts (gi_layout.h)
    DevBuf<TriGeom> d_tris;
    DevBuf<TriShade> d_shade;
    std::vector<uint32_t> tri_flags;      // TriGeom::flags of every entity, on the host: gi_lightmap_host refuses a chart row that names a sphere
    DevBuf<Mat> d_mats;
    std::vector<double> mat_roughness;    // Mat::roughness of every material, on the host: gi_render_baked_* picks each material's level of the chain from it
    DevBuf<LightD> d_lights;
    DevBuf<FogD> d_fogs;
    DevBuf<double> d_fog_grid;
    DevBuf<HaltonDim> d_hdims;            // the Halton tables are the context's own, uploaded once (gi_create)
    DevBuf<uint16_t> d_htable;

    // the laid-out scene to the device, and S pointed at it.  The fields of S that follow the switches are apply_switches's; the photon map stays
    // as it is: the reference keeps a valid map when the scene is edited and rebuilt (include/raytracer.h:56-72); RayTracer::setScene, which
    // allocates a fresh PhotonMap (include/raytracer.h:38), is gi_upload_scene + gi_clear_photons
    hipError_t upload(const HostScene& H, Scene& S)
    {
        hipError_t e = hipSuccess;
        auto up = [&e](auto& buf, const auto& v) { if (e == hipSuccess) e = buf.upload(v); };
        up(d_tnodes, H.tnodes); up(d_wnodes, H.wnodes); up(d_wleaf_id, H.wleaf_id); up(d_cboxes, H.cboxes); up(d_cuse, H.cuse);
        up(d_texs, H.texs); up(d_tri_uv, H.tri_uv); up(d_tex_pixels, H.tex_pixels); up(d_tex_lut, H.tex_lut);
        up(d_refs, H.refs); up(d_leaf_tris, H.leaf_tris); up(d_leaf_boxes, H.leaf_boxes); up(d_trace_boxes, H.trace_boxes);
        up(d_tcboxes, H.tcboxes); up(d_tcuse, H.tcuse);
        if (e != hipSuccess) return e;
        cuts = H.walk_cuts();
        up(d_tris, H.tris); up(d_shade, H.shade); up(d_mats, H.mats); up(d_lights, H.lights); up(d_fogs, H.fogs); up(d_fog_grid, H.fog_grid);
        if (e != hipSuccess) return e;
        tri_flags.resize(H.tris.size());
        for (size_t i = 0; i < H.tris.size(); i++) tri_flags[i] = H.tris[i].flags;
        mat_roughness.resize(H.mats.size());
        for (size_t i = 0; i < H.mats.size(); i++) mat_roughness[i] = H.mats[i].roughness;
        S.tnodes = d_tnodes.p; S.leaf_refs = d_refs.p; S.leaf_tris = d_leaf_tris.p; S.tris = d_tris.p; S.shade = d_shade.p;
        S.mats = d_mats.p; S.lights = d_lights.p;
        S.n_node = H.n_node; S.n_tri = H.n_tri; S.n_light = H.n_light;
        for (int k = 0; k < 3; k++) { S.root_bmin[k] = H.tnodes[0].bmin[k]; S.root_bmax[k] = H.tnodes[0].bmax[k]; }
        S.n_wnode = (int32_t)H.wnodes.size();
        S.wleaf_id = d_wleaf_id.p;
        S.cuse = d_cuse.p;
        S.tri_uv = d_tri_uv.p; S.texs = d_texs.p; S.tex_pixels = d_tex_pixels.p; S.tex_lut = d_tex_lut.p; S.n_tex = H.n_tex();
        S.has_spheres = 0;
        S.fogs = d_fogs.p; S.fog_grid = d_fog_grid.p; S.n_fog = H.n_fog();
        for (const TriGeom& g : H.tris) if (g.flags & 4u) S.has_spheres = 1;
        for (int k = 0; k < 3; k++) S.ambient[k] = H.ambient[k];
        have_scene = true;
        return hipSuccess;
    }
};

// ------------------------------------------------------------------------------------------------------------------------ the photon map
struct PhotonStore {
    DevBuf<PNode> d_pnodes;
    DevBuf<PRange> d_pranges;
    DevBuf<double> d_ph_pos, d_ph_dircol;
    int32_t n_prange = 0;             // entries of d_pranges in use
    bool pn_planes_ok = false;        // the uploaded photon octree qualifies for the one-record-per-level descent
    DevBuf<int32_t> d_pleaf_rank, d_prank_leaf, d_n_pleaf;   // build_photon_ranks
    DevBuf<uint32_t> d_pcand_off;                            // build_photon_candidates
    DevBuf<double> d_pcand, d_pcand_dc;
    DevBuf<PDescent> d_pdescent;                             // build_photon_descent
    DevBuf<int32_t> d_pjump;          // its jump table (gi_gather.h: gather_find_leaf_fast)
    DevBuf<double> d_pjump_aux;
    bool pdescent_ready = false, pjump_ready = false;   // d_pdescent / d_pjump hold the tables of the current photon map (apply_switches decides on their use)
};

// ------------------------------------------------------------------------------------------------------------------------ tuning
struct Tuning {
    bool flat_candidates = true;      // GI_FLAT_CANDIDATES=0: k_st_gather finds a leaf's k-th candidate through its range list, no k_st_gather_wave
    uint32_t gather_wave_below = 200000u;    // GI_GATHER_WAVE_BELOW: gather passes with fewer queries give every query a wave (k_st_gather_wave)
    bool fast_descent = true;         // GI_FAST_DESCENT=0: every gather query walks the full photon-octree records
    bool descent_jump = true;         // GI_DESCENT_JUMP=0: the fast descent of the gather keys starts at the root
    bool sort_cont = true;            // GI_SORT_CONT=0: continuing rays stay in queue order
    bool sort_shade = true;           // GI_SORT_SHADE=0: the shade stage takes a pass of continuing rays in the order the trace stage left them
    int sort_shade_lo = 5;            // GI_SORT_SHADE_LO: lowest slot bit that sort looks at (32 neighbouring records = 7 KB stay in the trace stage's order)
    int sort_lo_bit = 0;              // GI_SORT_LO_BIT: lowest key bit the sort of the continuing rays looks at (27-bit key: octant, 18 Morton bits, 6 direction bits)
    uint32_t refill_min = 32;         // GI_REFILL_MIN: idle lanes of a wave that make k_st_trace hand out new rays (64: lockstep waves)
    bool defer_shadows = true;        // GI_DEFER_SHADOWS=0: the shade kernel walks its shadow segments itself
    size_t lbuf_bytes_max = (size_t)16 << 30;   // GI_LBUF_MAX_BYTES: per-sample radiance buffer; frames beyond it run in sample chunks
    size_t pool_slots_max = (size_t)1 << 30;    // gi_set_pool_slots: upper bound on paths in flight; the actual pool is also bounded by free HBM (stream_samples)
    uint32_t finish_threshold = 1u << 17;   // GI_FINISH_THRESHOLD: paths left when the finisher takes over
    bool sample_identity = true;      // GI_SAMPLE_IDENTITY=0: the stream passes always keep the slot -> sample table, also where it would be the identity (stream_samples)
    bool keep_free_list = false;      // GI_KEEP_FREE_LIST=1: the stream passes write the free list in every pass, also where nothing will read it (trace_stage)
    bool early_miss = true;           // GI_EARLY_MISS: the deferred shade kernel ends a path whose next ray leaves the scene without meeting a leaf (passes_begin)
    uint32_t early_turns = 4;         // GI_EARLY_MISS_TURNS: turns of the walk that probe may take before it gives the ray to the trace stage
    uint32_t wave_factor = 0;         // GI_WAVE_FACTOR: finisher stages with at most this many paths per resident wave run one path per wave; 0 = by the size of the frame (passes_begin)
    uint32_t coop_factor = 4;         // GI_COOP_FACTOR: finisher stages with at most 4 x coop_factor x (resident waves) paths run one path per group of 16 lanes (at most 2 x: one per wave)
    // GI_FINISH_PLAN: finisher stages {paths per wave (0: spread evenly over the resident waves), max vertices}; the last stage runs to MAX_DEPTH.
    // Measured on the default frame (tools/stripe_probe.py): one full-wave stage 60 ms, this plan 51 ms; on 1/8 of the rows 40 -> 30 ms.
    std::vector<std::pair<int, int>> finish_plan = {{0, 1}, {0, 1}, {0, 1}, {0, 1}, {0, 2}, {0, 2}, {0, 4}, {0, 8}, {0, GI_MAX_DEPTH + 1}};

    static void env_flag(const char* name, bool& v) { if (const char* e = getenv(name)) v = atoi(e) != 0; }
    template <class T> static void env_int(const char* name, T& v, int lo, int hi) { if (const char* e = getenv(name)) v = (T)std::min(hi, std::max(lo, atoi(e))); }
    template <class T> static void env_size(const char* name, T& v, int base = 0, T cap = ~(T)0) { if (const char* e = getenv(name)) v = std::min<T>((T)strtoull(e, nullptr, base), cap); }
    static void env_plan(const char* name, std::vector<std::pair<int, int>>& v)   // "lanes:vertices,lanes:vertices,..."; anything else leaves the plan alone
    {
        const char* e = getenv(name);
        std::vector<std::pair<int, int>> plan;
        for (const char* q = e ? e : ""; *q;) {
            int l = 0, b = 0, used = 0;
            if (sscanf(q, "%d:%d%n", &l, &b, &used) != 2 || l < 0 || l > 64 || b < 1) { plan.clear(); break; }
            plan.push_back({l, b});
            q += used;
            if (*q == ',') q++;
        }
        if (!plan.empty()) v = plan;
    }
    // the context's tuning from the environment, and the three scene switches that have a variable
    static Tuning from_env(SceneSwitches& sw)
    {
        Tuning t;
        env_size("GI_LBUF_MAX_BYTES", t.lbuf_bytes_max);
        env_size("GI_COOP_FACTOR", t.coop_factor);
        env_size("GI_WAVE_FACTOR", t.wave_factor, 0, 0xffffu);
        env_flag("GI_EARLY_MISS", t.early_miss);
        env_int("GI_EARLY_MISS_TURNS", t.early_turns, 1, 64);
        env_flag("GI_SAMPLE_IDENTITY", t.sample_identity);
        env_flag("GI_KEEP_FREE_LIST", t.keep_free_list);
        env_flag("GI_SORT_CONT", t.sort_cont);
        env_flag("GI_DESCENT_JUMP", t.descent_jump);
        env_flag("GI_FLAT_CANDIDATES", t.flat_candidates);
        env_size("GI_GATHER_WAVE_BELOW", t.gather_wave_below, 10);
        env_flag("GI_SORT_SHADE", t.sort_shade);
        env_int("GI_SORT_SHADE_LO", t.sort_shade_lo, 0, INT_MAX);
        env_int("GI_SORT_LO_BIT", t.sort_lo_bit, 0, 26);
        env_flag("GI_DEFER_SHADOWS", t.defer_shadows);
        env_flag("GI_FAST_DESCENT", t.fast_descent);
        env_flag("GI_ENTITY_BOXES", sw.entity_boxes);
        env_flag("GI_CLIP_BOXES", sw.clip_boxes);
        env_flag("GI_WALK_CUT", sw.walk_cut);
        env_int("GI_REFILL_MIN", t.refill_min, 1, 64);
        env_size("GI_FINISH_THRESHOLD", t.finish_threshold);
        env_plan("GI_FINISH_PLAN", t.finish_plan);
        return t;
    }
};

// ------------------------------------------------------------------------------------------------------------------------ stage times
// stages of the per-stage device times (gi_last_kernel_ms; gi_last_stage_ms folds STG_SHADOW into STG_SHADE)
#define STG_COUNT_MAX 10
enum { STG_REGEN = 0, STG_TRACE, STG_SHADE, STG_SORT, STG_GATHER, STG_FINISH, STG_ACCUM, STG_OTHER, STG_SHADOW, STG_COUNT };

// Per-stage device time of the last streaming frame: a pair of HIP events around every timed stage, on the frame's stream; the pool of events
// grows with the longest frame and is kept.  The sums are computed once per frame: the runtime's answer for one pair of events is not the same
// number at every call (it was seen to move by a nanosecond between two calls with nothing recorded in between), and a time that nothing has
// touched must read the same.
struct StageClock {
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_stage;        // stage id of event pair k (events 2k, 2k+1)
    size_t ev_used = 0;
    bool stage_timing = true;
    bool summed = false;              // stage_ms holds the sums of the pairs recorded so far: read() has nothing to do
    float stage_ms[STG_COUNT_MAX] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    StageClock() = default;
    StageClock(const StageClock&) = delete;
    StageClock& operator=(const StageClock&) = delete;
    ~StageClock() { for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e); }
    void restart() { ev_used = 0; ev_stage.clear(); summed = false; }   // a new frame
    void begin(int stage, hipStream_t st)
    {
        if (!stage_timing) return;
        if (ev_used + 2 > ev_pool.size()) {
            for (int k = 0; k < 2; k++) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ev_pool.push_back(e); }
        }
        ev_stage.push_back(stage);
        summed = false;
        (void)hipEventRecord(ev_pool[ev_used], st);
    }
    void end(hipStream_t st)
    {
        if (!stage_timing || ev_used + 2 > ev_pool.size()) return;
        (void)hipEventRecord(ev_pool[ev_used + 1], st);
        ev_used += 2;
    }
    // stage_ms = the sums of the pairs recorded since restart(); debug: a "[stage]" line per pair (GI_DEBUG_STAGES)
    // (kept once every pair has answered; a pair that is not ready yet is asked again at the next call)
    void read(bool debug)
    {
        if (summed && !debug) return;
        for (int k = 0; k < STG_COUNT_MAX; k++) stage_ms[k] = 0;
        const size_t n_pairs = std::min({ev_used / 2, ev_stage.size(), ev_pool.size() / 2});
        bool all = true;
        for (size_t k = 0; k < n_pairs; k++) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev_pool[2 * k], ev_pool[2 * k + 1]) == hipSuccess) stage_ms[ev_stage[k]] += t;
            else all = false;
            if (debug) fprintf(stderr, "[stage] %d %.3f ms\n", ev_stage[k], t);
        }
        summed = all;
    }
};

// ------------------------------------------------------------------------------------------------------------------------ stream workspaces
struct StreamGrids { int lds_refused = 0; int pix = 0, trace = 0, shade = 0, shadow = 0, gather = 0, accum = 0, finish = 0, ad_gen = 0, ad_accum = 0, compact = 0; };

// Workspaces of the stream passes, in 32-bit words, grown on demand for P paths in flight and kept between frames (stream_alloc, kStreamWork).
// A name after `&` is a second role of the buffer it refers to.  The roles of one buffer cannot overlap in time because every launch of a pass goes
// to the context's one stream in the order of kPassStages: the trace stage's staging queues are read by its compaction before the shade kernel
// appends to them again; the shade sort's iota, sorted queue and places are last read by the shade kernel, and the compaction behind that kernel
// is the first to write the gather queries into the same buffers, which the gather of this pass reads before the next pass sorts its shade queue.
struct StreamWork {
    using Buf = DevBuf<uint32_t>;
    Buf q_new;                                        // paths a round prepared (k_ad_gen); the refill of a chunk starts its samples in the trace kernel
    Buf q_cont_a, q_cont_b;                           // continuing rays in coherence order: a pass reads one (in) while its last sort fills the other (out)
    Buf q_shade;                                      // hits of the trace stage
    Buf q_gather;                                     // no reader at present (the gather queries go straight to gather_slots / gather_keys); part of the budget
    Buf q_free_a, q_free_b;                           // freed slots: written by a pass (out), handed to new samples by the refill of the next (in)
    Buf gather_keys, gather_slots;                    // the gather queries of a pass in queue order: photon-map leaf, path slot
    Buf gather_keys_sorted, gather_slots_sorted;      // ... in leaf order
    Buf& shade_iota = gather_slots;                   // the shade sort: 0, 1, 2, ...
    Buf& shade_sorted = gather_keys_sorted;           //   the shade queue in slot order
    Buf& shade_places = gather_slots_sorted;          //   where each item stood in the trace stage's order
    Buf cont_keys, cont_keys_sorted;                  // coherence keys of the continuing rays
    Buf stage_hits, stage_free_trace;                 // staging queues the producers append to, one segment per workgroup (k_st_compact closes the gaps): trace stage
    Buf& stage_cont_slots = stage_hits;               //   shade stage: continuing slot
    Buf& stage_cont_keys = stage_free_trace;          //   its coherence key
    Buf stage_gather_slots, stage_free_shade;         //   gather slot, freed slot
    Buf stage_gather_pos;                             //   gather position (3 doubles per entry)
    Buf cont_slots;                                   // continuing slots in queue order
    Buf sort_scratch;                                 // gi_sort.inc ping-pongs through one more copy of keys and values (sort_pairs)
};
// what stream_alloc gives every workspace, in words: per path slot, and on top of that.  Staging segments are laid out as if every chunk of a
// producer's loop were full: up to one chunk of slack.
struct StreamWorkItem { StreamWork::Buf StreamWork::* buf; uint32_t per_slot, fixed; };
static constexpr StreamWorkItem kStreamWork[] = {
    {&StreamWork::q_new, 1, 0}, {&StreamWork::q_cont_a, 1, 0}, {&StreamWork::q_cont_b, 1, 0}, {&StreamWork::q_shade, 1, 0}, {&StreamWork::q_gather, 1, 0},
    {&StreamWork::q_free_a, 1, 0}, {&StreamWork::q_free_b, 1, 0},
    {&StreamWork::gather_keys, 1, 0}, {&StreamWork::gather_slots, 1, 0}, {&StreamWork::gather_keys_sorted, 1, 0}, {&StreamWork::gather_slots_sorted, 1, 0},
    {&StreamWork::cont_keys, 1, 0}, {&StreamWork::cont_keys_sorted, 1, 0},
    {&StreamWork::stage_hits, 1, 4096}, {&StreamWork::stage_free_trace, 1, 4096}, {&StreamWork::stage_gather_slots, 1, 4096}, {&StreamWork::stage_free_shade, 1, 4096},
    {&StreamWork::stage_gather_pos, 6, 6 * 4096},
    {&StreamWork::cont_slots, 1, 0}, {&StreamWork::sort_scratch, 2, 0}};
constexpr size_t stream_work_bytes_per_slot()
{
    size_t words = 0;
    for (const StreamWorkItem& w : kStreamWork) words += w.per_slot;
    return words * sizeof(uint32_t);
}
// the pool is sized from gi_layout.h's budget per slot (plan_pool): a workspace added here without a term there would overcommit memory
static_assert(stream_work_bytes_per_slot() + sizeof(unsigned long long) /* d_slot_sample */ <= kBudgetWorkBytes, "kStreamWork allocates more per slot than plan_pool budgets");

// the field arrays of a pool of n paths in one allocation (StreamState::d_spool)
static PathPool make_path_pool(void* base, size_t n)
{
    PathPool P;
    char* b = static_cast<char*>(base);
    P.ray = reinterpret_cast<PoolRay*>(b); b += n * sizeof(PoolRay);
    P.hit = reinterpret_cast<PoolHit*>(b); b += n * sizeof(PoolHit);
    P.thru = reinterpret_cast<PoolThru*>(b); b += n * sizeof(PoolThru);
    P.gath = reinterpret_cast<PoolGath*>(b); b += n * sizeof(PoolGath);
    P.L = reinterpret_cast<double*>(b);
    return P;
}

// Everything the schedules keep on the device between frames (grown on demand), and the two pinned mirrors they read back through.
struct StreamState {
    StreamGrids grids;                    // launch grids of the streaming kernels on this context's device (stream_grids)
    StreamWork work;                      // queues, keys and scratch of the stream passes
    DevBuf<unsigned char> d_spool;        // paths of the streaming pipeline: field arrays (PathPool), GI_POOL_BYTES_PER_SLOT each
    size_t spool_slots = 0;
    DevBuf<unsigned long long> d_slot_sample;
    DevBuf<double> d_lbuf;                // per-sample radiance of the current chunk or round
    DevBuf<PixRec> d_pix;                 // pixel records of a one-shot frame
    DevBuf<uint32_t> d_pixtab;            // k_pixel_table of the frame being rendered
    DevBuf<StreamCtl> d_ctl;
    PinnedBuf<StreamCtl> h_ctl;           // the totals of a pass, read back behind the shade stage
    DevBuf<unsigned int> d_wfcnt;         // rounds (run_rounds): [0] paths started by k_ad_gen, [1] pixels still wanting samples
    PinnedBuf<unsigned int> h_wfcnt;      // host mirror of d_wfcnt
    DevBuf<ShadowQ> d_shq;                // shadow queries the shade stage put off (one light, wide records): entry i belongs to item i of the shade queue
    DevBuf<unsigned int> d_blkcnt;        // per-workgroup append counters [QC_KINDS][GI_MAX_PRODUCER_BLOCKS], 128 bytes apart
    DevBuf<uint32_t> d_segs;              // segment start of every producer workgroup
    DevBuf<uint32_t> d_rs_hist;           // gi_sort.inc: [digit][workgroup] counters of a radix pass
    bool rs_attr_set = false;
    DevBuf<unsigned int> d_fin_cnt;       // survivors of every finisher stage (finish_tail)
    DevBuf<StreamCounters> d_stream_cnt;  // gi_set_counters(ctx, 2)
    DevBuf<unsigned int> d_tile_counter;  // the megakernel's tile dealer and its counters (gi_set_counters(ctx, 1))
    DevBuf<Counters> d_counters;

    // everything the pass loop needs for P paths in flight (the radiance buffer is the caller's); n_shadow: deferred shadow queries per path
    // need_table: the caller's passes read slot_sample (sample_of); a chunk whose samples are all in flight at once does without it
    hipError_t alloc(uint32_t P, bool need_table, int n_shadow);   // gi_stream.inc, behind the sort's constants
    // Bytes of the above that the context holds already and the next frame would re-use (plan_pool: held_b): pool, radiance buffer, shadow queries and
    // queues.  The queues are an estimate: q_new and q_free_b each stand for 7 workspaces of their size, 4 bytes an entry (the queues were two
    // families of seven when the term was written).  kStreamWork holds more words per slot today; counting less as held only plans a smaller pool.
    size_t held_bytes() const { return d_spool.n + d_lbuf.n * 8 + (work.q_new.n + work.q_free_b.n) * 4 * 7 + d_shq.n * sizeof(ShadowQ); }
};

// ------------------------------------------------------------------------------------------------------------------------ auxiliary passes
// An auxiliary pass keeps a timer of its own, so it leaves the frame's times (t_frame, StageClock) alone; lds_refused: -1 = its kernel instances
// were not asked for their LDS yet, else as StreamGrids::lds_refused.
struct AuxPass {
    EventTimer timer;
    int lds_refused = -1;
};
// the denoiser, with its scratch: the guide records [h][w][8] and two colour buffers [h][w][3], f64, sized on first use and kept (dn_reserve,
// gi_denoise.inc); the upsampler packs its low frame there too
struct DenoisePass : AuxPass {
    DevBuf<double> d_guides, d_a, d_b;
};
// a bake (gi_bake.inc), with what it keeps beside the stream workspaces: every path's unit direction [slot][3] (probes: the fold's basis is
// evaluated there) and the sums of a chunk's points between two ranges of samples [terms][points], f64, sized on first use and kept
struct BakePass : AuxPass {
    DevBuf<double> d_dirs, d_sums;
};
// a lightmap (gi_lightmap.inc): the stage timers beside the pass's own, and its scratch, sized on first use and kept.  work [6 T] f64 holds the
// texels' points until they are compacted and the two dilation buffers [T][3] after the bake
struct LightmapPass : AuxPass {
    EventTimer t_stage[3];            // raster + rank, bake, scatter + dilate
    DevBuf<int32_t> d_own, d_texel;   // [T] owner row (the raster's atomicMin table, then -1 where not covered); [n_cov] texel of a table row
    DevBuf<uint32_t> d_rank, d_blk;   // [T] row of a covered texel; covered texels per workgroup, scanned
    DevBuf<double> d_work, d_points, d_rows;   // d_points [n_cov][6], d_rows [n_cov][3]: the bake's input and output
    DevBuf<unsigned char> d_fill;     // [2][T] filled flags of the two dilation buffers
};
// a reflection probe (gi_cubemap.inc): the stage timers beside the pass's own, and its scratch, sized on first use and kept: the capture B_0
// [6 N^2][3], the box levels 1 .. levels - 2 behind one another, and the prefilter's partial sums [6][6 (N / 2)^2][4], all f64
struct CubemapPass : AuxPass {
    EventTimer t_stage[2];            // capture, prefilter
    DevBuf<double> d_b0, d_box, d_part;
};
// the baked-light pass (gi_baked.inc): the level of the chain every material reads [n_mat], made per call, sized on first use and kept; with a
// lightmap (gi_render_baked_lightmap_*) also the chart row that serves every entity [n_tri], the call's LitLm, and lm_lds_refused: lds_refused of
// the LM instances
struct LitLm;
struct LitPass : AuxPass {
    DevBuf<int32_t> d_levels;
    DevBuf<int> d_lm_rows;
    DevBuf<LitLm> d_lm;
    int lm_lds_refused = -1;
    int pv_lds_refused = -1;          // lds_refused of the PV instances (gi_render_baked_visibility_*)
    int rs_lds_refused = -1;          // lds_refused of the RS instances (gi_render_baked_reflections_*)
};
// the final-gather pass (gi_finalgather.inc): a timer, an LDS answer and a level table of its own [n_mat], made per call with a chain, sized on
// first use and kept -- the baked-light pass's are left alone
struct FgPass : AuxPass {
    DevBuf<int32_t> d_levels;
};

// ------------------------------------------------------------------------------------------------------------------------ the context
struct gi_ctx {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    std::string err;
    Scene S{};                        // what the kernels get: pointers into scene and photons, set by their functions and by apply_switches
    SceneSwitches sw;                 // gi_set_wide_nodes, gi_set_content_culling, gi_set_entity_boxes, GI_ENTITY_BOXES, GI_CLIP_BOXES, GI_WALK_CUT
    int render_mode = 0;              // 0 streaming passes (fixed spp) or rounds (adaptive), 1 megakernel, 2 synchronous rounds always (gi_set_render_mode)
    EventTimer t_frame;               // around the kernels of the last gi_render_* / gi_progressive_step_* call
    int last_launches = 0;
    bool count_enabled = false;       // gi_set_counters(ctx, 1): the megakernel counts the reference's visits (per-node walk)
    bool count_stream = false;        // gi_set_counters(ctx, 2): the streaming kernels count what they execute (StreamCounters)
    unsigned long long stream_shaded = 0;   // shaded hits of the last counted frame (sum of the shade queues' lengths)
    Counters last_counters{};
    // a progressive session (gi_progressive_*): the pixel records it owns between steps -- everything else a step uses is the shared state below
    struct Progressive {
        bool open = false;
        gi_render_params rp{};
        Frame F{};                    // make_frame(rp): max_samples is the session's own
        int schedule = 0;             // 0: refill pipeline, records in st_pixel_xy order; 1: synchronous rounds, records in padded 8x8 tiles (tile_pixel_xy)
        int32_t sample_end = 0;       // E: every pixel has been offered samples [0, E)
        uint32_t n_rec = 0;
        DevBuf<PixRec> pix;
    } prog;
    SceneStore scene;
    PhotonStore photons;
    Tuning tune;
    StageClock clock;
    StreamState st;
    // the thin lens (gi_set_lens): what the caller set, and the aperture's vertices on the device.  S.lens_* follow it (set_lens, gi_lens.inc);
    // uploads of scenes and photons leave them alone
    struct LensState {
        gi_lens lens{0.0, 0.0, 6, 0};
        DevBuf<double> d_verts;       // [GI_LENS_MAX_BLADES + 1][2], allocated by the first lens with a radius
    } lens;
    AuxPass feat, ao, up;             // gi_render_features_*, gi_render_occlusion_*, gi_upsample_*
    LitPass lit;                      // gi_render_baked_*
    FgPass fg;                        // gi_render_final_gather_*
    DenoisePass dn;                   // gi_denoise_*
    BakePass bake;                    // gi_bake_*
    LightmapPass lm;                  // gi_lightmap_*
    CubemapPass cm;                   // gi_cubemap_*
    AuxPass pv;                       // gi_probe_visibility_*
};

namespace {

int fail(gi_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

// gi_last_<pass>_ms: the device time of the pass's last call (EventTimer::read)
template <class Pass> int pass_ms(gi_ctx* c, Pass gi_ctx::*pass, float* ms)
{
    if (!c || !ms) return GI_E_INVALID;
    HIP_TRY(c, (c->*pass).timer.read(ms));
    return GI_OK;
}

// The device side of a host-pointer entry, after its argument and state checks.  in() uploads a caller's array, out() allocates a
// result and notes where it goes (h == nullptr: an optional output nobody asked for -- the kernel still writes it), scratch() is memory of this
// call alone; each takes the element count, once.  run(launch) launches (unless a buffer failed), asks for the launch's status, waits for the
// stream and copies the results back in the order of the out() calls.  launch returns nothing, or a failure it has recorded with fail().
// timer: the pass's, where the launch is a timed pass (finish_to_host: a call that fails at its end has no time to report).
struct Entry {
    gi_ctx* c;
    const char* what;
    EventTimer* timer;
    hipError_t e;
    DevBuf<unsigned char> buf[16];
    ToHost outs[6];
    int n_buf = 0, n_out = 0;
    Entry(gi_ctx* c_, const char* what_, EventTimer* timer_ = nullptr) : c(c_), what(what_), timer(timer_), e(hipSetDevice(c_->device)) {}
    template <class T> T* scratch(size_t count)
    {
        if (e == hipSuccess) e = n_buf < 16 ? buf[n_buf].alloc(count * sizeof(T)) : hipErrorOutOfMemory;
        return e == hipSuccess ? reinterpret_cast<T*>(buf[n_buf++].p) : nullptr;
    }
    template <class T> const T* in(const T* h, size_t count)
    {
        if (e == hipSuccess) e = n_buf < 16 ? buf[n_buf].upload(reinterpret_cast<const unsigned char*>(h), count * sizeof(T)) : hipErrorOutOfMemory;
        return e == hipSuccess ? reinterpret_cast<const T*>(buf[n_buf++].p) : nullptr;
    }
    template <class T> T* out(T* h, size_t count)
    {
        T* d = scratch<T>(count);
        if (d && n_out == 6) e = hipErrorOutOfMemory;
        if (e == hipSuccess) outs[n_out++] = ToHost{h, d, count * sizeof(T)};
        return d;
    }
    template <class Launch> int run(Launch launch)
    {
        if (e == hipSuccess) {
            if constexpr (std::is_void<decltype(launch())>::value) launch();
            else if (const int rc = launch()) return rc;
            e = hipGetLastError();
        }
        if (e != hipSuccess) return fail(c, GI_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
        return finish_to_host(c, what, outs, (size_t)n_out, timer);
    }
};

}  // namespace

__global__ __launch_bounds__(1024) void k_rs_scan(uint32_t* ghist, uint32_t total);   // gi_sort.inc
// The Scene fields that follow the context's switches, from the uploaded tables and the switches alone (gi_layout.h: apply_scene_switches, which
// the CPU suite's emulator calls too).  Every upload, every change of the photon map and every gi_set_* of a switch ends here, and nothing else
// assigns these fields.
static void apply_switches(gi_ctx* c)
{
    const SceneStore& s = c->scene;
    const PhotonStore& ph = c->photons;
    SceneTables T;
    T.wnodes = s.d_wnodes.p; T.cboxes = s.d_cboxes.p; T.n_cboxes = s.d_cboxes.n;
    T.leaf_boxes = s.d_leaf_boxes.p; T.trace_boxes = s.d_trace_boxes.p;
    T.tcboxes = s.d_tcboxes.p; T.n_tcboxes = s.d_tcboxes.n; T.tcuse = s.d_tcuse.p;
    T.set_walk_cuts(s.cuts);
    T.pn_planes_ok = ph.pn_planes_ok;
    T.pdescent = ph.pdescent_ready ? ph.d_pdescent.p : nullptr;
    T.pjump = ph.pjump_ready ? ph.d_pjump.p : nullptr;
    apply_scene_switches(c->S, T, c->sw);
}

// ---- the tables derived from the photon map c->S points at, in the order install_photon_map builds them
// the sort key of the gather queries: every leaf's rank (k_pleaf_rank), and the number of leaves
static int build_photon_ranks(gi_ctx* c)
{
    Scene& S = c->S;
    PhotonStore& ph = c->photons;
    if (ph.d_pleaf_rank.n < (size_t)S.n_pnode) { HIP_TRY(c, ph.d_pleaf_rank.alloc((size_t)S.n_pnode)); HIP_TRY(c, ph.d_prank_leaf.alloc((size_t)S.n_pnode)); }
    if (!ph.d_n_pleaf.p) HIP_TRY(c, ph.d_n_pleaf.alloc(1));
    hipLaunchKernelGGL(k_pleaf_rank, dim3(1), dim3(1024), 0, c->stream, S.pnodes, S.n_pnode, ph.d_pleaf_rank.p, ph.d_prank_leaf.p, ph.d_n_pleaf.p);
    HIP_TRY(c, hipGetLastError());
    int32_t n = 0;
    HIP_TRY(c, hipMemcpyAsync(&n, ph.d_n_pleaf.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    S.pleaf_rank = ph.d_pleaf_rank.p; S.prank_leaf = ph.d_prank_leaf.p; S.n_pleaf = n;
    return GI_OK;
}
// the leaves' candidate lists, written out flat (GI_FLAT_CANDIDATES): offsets by a count and a scan, then the candidates
static int build_photon_candidates(gi_ctx* c)
{
    Scene& S = c->S;
    PhotonStore& ph = c->photons;
    const int32_t n = S.n_pleaf;
    if (!(c->tune.flat_candidates && n > 0)) return GI_OK;
    if (ph.d_pcand_off.n < (size_t)n + 1) HIP_TRY(c, ph.d_pcand_off.alloc((size_t)n + 1));
    hipLaunchKernelGGL(k_pcand_count, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, c->stream, S.pnodes, ph.d_prank_leaf.p, n, ph.d_pcand_off.p);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, c->stream, ph.d_pcand_off.p, (uint32_t)n + 1u);
    HIP_TRY(c, hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, ph.d_pcand_off.p + n, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!(total > 0 && total < 0x7fffffffu)) return GI_OK;
    if (ph.d_pcand.n < (size_t)total * 3) { HIP_TRY(c, ph.d_pcand.alloc((size_t)total * 3)); HIP_TRY(c, ph.d_pcand_dc.alloc((size_t)total * 6)); }
    hipLaunchKernelGGL(k_pcand_fill, dim3(1024), dim3(256), 0, c->stream, S.pnodes, S.pranges, S.ph_pos, S.ph_dircol, ph.d_prank_leaf.p, n, ph.d_pcand_off.p, ph.d_pcand.p, ph.d_pcand_dc.p);
    HIP_TRY(c, hipGetLastError());
    S.pcand_off = ph.d_pcand_off.p; S.pcand = ph.d_pcand.p; S.pcand_dc = ph.d_pcand_dc.p;
    return GI_OK;
}
// the jump table of the fast descent over the map's box `root` (GI_DESCENT_JUMP): the cell a position falls in names the record its descent starts at
static int build_photon_jump(gi_ctx* c, const PNode& root)
{
    Scene& S = c->S;
    PhotonStore& ph = c->photons;
    const size_t n_cells = (size_t)GI_PJUMP_N * GI_PJUMP_N * GI_PJUMP_N;
    double ext = 0.0, host[7];
    for (int k = 0; k < 3; k++) { ext = std::max(ext, root.bmax[k] - root.bmin[k]); S.pjump_cell[k] = (root.bmax[k] - root.bmin[k]) / (double)GI_PJUMP_N; S.pjump_inv[k] = (double)GI_PJUMP_N / (root.bmax[k] - root.bmin[k]); }
    bool ok = ext > 0.0;
    for (int k = 0; k < 3; k++) { host[k] = root.bmin[k]; host[3 + k] = S.pjump_cell[k]; if (!(S.pjump_cell[k] > 0.0) || !std::isfinite(S.pjump_inv[k])) ok = false; }
    if (!ok) return GI_OK;
    if (ph.d_pjump.n < n_cells) HIP_TRY(c, ph.d_pjump.alloc(n_cells));
    if (ph.d_pjump_aux.n < 8) HIP_TRY(c, ph.d_pjump_aux.alloc(8));
    host[6] = 0.0;                                                    // (as an int: the "bad" flag)
    HIP_TRY(c, hipMemcpyAsync(ph.d_pjump_aux.p, host, sizeof host, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pjump, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, c->stream, ph.d_pdescent.p, ph.d_pjump_aux.p, ph.d_pjump_aux.p + 3, 1e-12 * ext, ph.d_pjump.p, reinterpret_cast<int*>(ph.d_pjump_aux.p + 6));
    HIP_TRY(c, hipGetLastError());
    int bad = 1;
    HIP_TRY(c, hipMemcpyAsync(&bad, ph.d_pjump_aux.p + 6, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ph.pjump_ready = !bad;
    return GI_OK;
}
// the split records of the descent and the map's own box (gather_find_leaf_fast), for a map that qualifies whatever the switches are now: the
// one-record-per-level layout only (children from the parent's planes); then the jump table
static int build_photon_descent(gi_ctx* c)
{
    Scene& S = c->S;
    PhotonStore& ph = c->photons;
    if (!(c->tune.fast_descent && ph.pn_planes_ok)) return GI_OK;
    if (ph.d_pdescent.n < (size_t)S.n_pnode) HIP_TRY(c, ph.d_pdescent.alloc((size_t)S.n_pnode));
    hipLaunchKernelGGL(k_pdescent, dim3((unsigned)((S.n_pnode + 255) / 256)), dim3(256), 0, c->stream, S.pnodes, S.n_pnode, ph.d_pdescent.p);
    HIP_TRY(c, hipGetLastError());
    PNode root;
    HIP_TRY(c, hipMemcpyAsync(&root, S.pnodes, sizeof(PNode), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; k++) { S.pmap_bmin[k] = root.bmin[k]; S.pmap_bmax[k] = root.bmax[k]; }
    ph.pdescent_ready = true;
    return c->tune.descent_jump ? build_photon_jump(c, root) : GI_OK;
}

// A photon map now in d_pnodes / d_pranges / d_ph_pos / d_ph_dircol (gi_upload_photons, build_photon_map_on_device): the scene reads it from
// there, and its tables are built: ranks, candidates, descent
static int install_photon_map(gi_ctx* c, int32_t n_node, int32_t n_photon, int32_t n_prange, bool planes_ok)
{
    Scene& S = c->S;
    PhotonStore& ph = c->photons;
    S.pnodes = ph.d_pnodes.p; S.pranges = ph.d_pranges.p; S.ph_pos = ph.d_ph_pos.p; S.ph_dircol = ph.d_ph_dircol.p;
    S.n_pnode = n_node; S.n_photon = n_photon;
    ph.n_prange = n_prange;
    ph.pn_planes_ok = planes_ok;
    S.pleaf_rank = nullptr; S.prank_leaf = nullptr; S.n_pleaf = 0; S.pcand_off = nullptr; S.pcand = nullptr; S.pcand_dc = nullptr;
    ph.pdescent_ready = false; ph.pjump_ready = false;
    int rc = GI_OK;
    if (S.n_pnode > 0) {
        rc = build_photon_ranks(c);
        if (rc == GI_OK) rc = build_photon_candidates(c);
        if (rc == GI_OK) rc = build_photon_descent(c);
    }
    apply_switches(c);
    return rc;
}

// no photon map (a fresh PhotonMap): gather queries find nothing
static void clear_photon_map(gi_ctx* c)
{
    Scene& S = c->S;
    S.pnodes = nullptr; S.ph_pos = nullptr; S.ph_dircol = nullptr; S.n_pnode = 0; S.n_photon = 0; S.n_pleaf = 0;
    c->photons.pdescent_ready = false; c->photons.pjump_ready = false;
    apply_switches(c);
}
