// gi_stream.inc -- the host side of the streaming pipeline: which k_st_* kernel runs when, on which queue.  Host code only; the kernels are
// gi_stages.inc's and gi_pixels.inc's, their instance tables and selectors (st_trace, st_shade, ...) gi_instances.inc's, the workspaces (StreamState, StreamWork,
// kStreamWork) and the stage clock gi_context.inc's.  Included by gi_kernels.hip behind gi_sort.inc; the render entries that choose between the
// schedules are in gi_api.inc.
//
//   stream_samples   fixed sample count: chunks of samples through the pool, freed slots refilled with the next samples (ChunkRefill)
//   run_rounds       adaptive sampling and render mode 2: synchronous rounds, k_ad_gen prepares the paths of a round (RoundRefill)
//   stream_passes    the pass loop both run: kPassStages in order, until few enough paths are left for the finisher (finish_tail)
//   plan_pool        (gi_layout.h) how many paths are in flight: the memory budget per slot, which kStreamWork (gi_context.inc) must stay within
static int grid_for(gi_ctx* c, const void* kernel, size_t dyn_lds = 0, int block = GI_BLOCK)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, dyn_lds) != hipSuccess || per_cu <= 0) per_cu = 1;
    return c->n_cu * per_cu;
}

static int render_megakernel(gi_ctx* c, const Frame& F, void* d_out, int out_is_f64, int32_t* d_spp)
{
    HIP_TRY(c, hipMemsetAsync(c->st.d_tile_counter.p, 0, sizeof(unsigned int), c->stream));
    if (c->count_enabled) HIP_TRY(c, hipMemsetAsync(c->st.d_counters.p, 0, sizeof(Counters), c->stream));
    const int grid = c->n_cu * 2;
    HIP_TRY(c, c->t_frame.begin(c->stream));
    if (c->count_enabled)
        hipLaunchKernelGGL(k_render<true>, dim3(grid), dim3(GI_BLOCK), 0, c->stream, c->S, F, d_out, out_is_f64, d_spp, c->st.d_tile_counter.p, c->st.d_counters.p);
    else
        hipLaunchKernelGGL(k_render<false>, dim3(grid), dim3(GI_BLOCK), 0, c->stream, c->S, F, d_out, out_is_f64, d_spp, c->st.d_tile_counter.p, c->st.d_counters.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->t_frame.end(c->stream));
    c->last_launches = 1;
    return GI_OK;
}

// One timed stage of a frame: an event pair around its launches, and every launch counted where it is made (n_launches of gi_last_render_ms).
struct TimedStage {
    gi_ctx* c;
    int& launches;
    TimedStage(gi_ctx* c_, int stage, int& launches_) : c(c_), launches(launches_) { c->clock.begin(stage, c->stream); }
    ~TimedStage() { c->clock.end(c->stream); }
    template <class K, class... A> void launch(K kernel, dim3 grid, dim3 block, size_t lds, const A&... args)
    {
        hipLaunchKernelGGL(kernel, grid, block, lds, c->stream, args...);
        launches++;
    }
};

static const StreamGrids& stream_grids(gi_ctx* c)   // per context: one process may drive several devices (gi_group_*)
{
    StreamGrids& g = c->st.grids;
    if (!g.trace) {
        auto grid_of = [&](const auto& k, int block) { return grid_for(c, (const void*)k.fn, k.lds, block); };
        ask_for_lds(kTrace, g.lds_refused); ask_for_lds(kShade, g.lds_refused); ask_for_lds(kShadow, g.lds_refused); ask_for_lds(kFinish, g.lds_refused);
        g.pix = grid_for(c, (const void*)k_pix_init); g.trace = grid_of(st_trace(7, true, false, false), GI_TRACE_BLOCK);
        g.shade = grid_of(st_shade(7, true, 0), GI_SHADE_BLOCK); g.shadow = grid_of(st_shadow(7, true, false), GI_SHADOW_BLOCK); g.gather = grid_for(c, (const void*)st_gather(false)); g.accum = grid_for(c, (const void*)k_st_accum);
        g.compact = grid_for(c, (const void*)k_st_compact, 0, 256); g.finish = grid_of(st_finish(7, true, 0), GI_FINISH_BLOCK); g.ad_gen = grid_for(c, (const void*)k_ad_gen); g.ad_accum = grid_for(c, (const void*)k_ad_accum);
    }
    return g;
}
// The gather of a pass (gather_stage, gi_debug_gather_pass): n queries in leaf order (keys, vals = their slots), the caustic term added to their
// radiance in lbuf; a wave per query (k_st_gather_wave) or a lane per query (k_st_gather)
static int photon_key_bits(const Scene& S)   // of the gather queries' sort key: a leaf's rank, 0 .. n_pleaf
{
    int bits = 1;
    while ((1u << bits) <= (uint32_t)S.n_pleaf) bits++;
    return bits;
}
static void launch_gather(gi_ctx* c, bool wave, bool counting, const PathPool& pool, const uint32_t* keys, const uint32_t* vals, uint32_t n,
                          const unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, StreamCounters* sc)
{
    if (wave)
        hipLaunchKernelGGL(st_gather_wave(counting), dim3(std::min<uint32_t>((uint32_t)(5 * c->n_cu), (n + 3u) / 4u)), dim3(GI_GW_BLOCK), 0, c->stream, c->S, pool, keys, vals, n, slot_sample, sample0, lbuf, sc);
    else
        hipLaunchKernelGGL(st_gather(counting), dim3(stream_grids(c).gather), dim3(GI_BLOCK), 0, c->stream, c->S, pool, keys, vals, n, slot_sample, sample0, lbuf, sc);
}
// a few lights, wide records: the shadow walks of the shade stage run in a kernel of their own (ShadowQ)
static bool defers_shadows(const gi_ctx* c) { return c->tune.defer_shadows && c->S.wnodes != nullptr && c->S.n_light >= 1 && c->S.n_light <= 4; }   // one query per light and shaded hit

hipError_t StreamState::alloc(uint32_t P, bool need_table, int n_shadow)
{
    hipError_t e = hipSuccess;
    auto grow = [&e](auto& buf, size_t need) { if (e == hipSuccess && buf.n < need) e = buf.alloc(need); };
    auto once = [&e](auto& buf, size_t count) { if (e == hipSuccess && !buf.p) e = buf.alloc(count); };
    if (spool_slots < P) { grow(d_spool, (size_t)P * GI_POOL_BYTES_PER_SLOT); if (e == hipSuccess) spool_slots = P; }
    if (need_table) grow(d_slot_sample, P);
    for (const StreamWorkItem& w : kStreamWork) grow(work.*w.buf, (size_t)P * w.per_slot + w.fixed);
    grow(d_shq, (size_t)P * (size_t)n_shadow);
    once(d_blkcnt, (size_t)QC_KINDS * GI_MAX_PRODUCER_BLOCKS * GI_CNT_STRIDE);
    once(d_segs, GI_MAX_PRODUCER_BLOCKS);
    once(d_rs_hist, (size_t)GI_RS_MAXBINS * GI_MAX_PRODUCER_BLOCKS);
    once(d_ctl, 1);
    once(h_ctl, 1);
    return e;
}
static int stream_alloc(gi_ctx* c, uint32_t P, bool need_table)
{
    HIP_TRY(c, c->st.alloc(P, need_table, defers_shadows(c) ? c->S.n_light : 0));
    return GI_OK;
}
// ---- the new paths of a pass.  A schedule's refill is asked once per pass, with the slots the pass before freed (q_free == nullptr: slots
// 0 .. n_free - 1), and answers with everything the pass needs to know: paths it has prepared in work.q_new, samples the trace kernel is to start
// itself (gen.n_gen of them), and whether it will start no more after these.
struct NewPaths { uint32_t n_prepared; GenArgs gen; bool exhausted; };
struct Refill {
    virtual NewPaths next(uint32_t n_free, const uint32_t* q_free) = 0;
protected:
    ~Refill() = default;
};
// path regeneration (stream_samples): free slots take the next samples of the chunk [sample0, sample_end), which starts at sample s0 of every pixel
struct ChunkRefill final : Refill {
    const Frame& F;
    const uint32_t* pixtab;
    uint32_t n_pix;
    int s0;
    unsigned long long sample0, sample_end, next_sample;
    ChunkRefill(const Frame& F_, const uint32_t* pixtab_, uint32_t n_pix_, int s0_, int ns)
        : F(F_), pixtab(pixtab_), n_pix(n_pix_), s0(s0_), sample0((unsigned long long)s0_ * n_pix_), sample_end((unsigned long long)(s0_ + ns) * n_pix_), next_sample(sample0) {}
    NewPaths next(uint32_t n_free, const uint32_t* q_free) override
    {
        NewPaths nw;
        memset(&nw, 0, sizeof nw);                     // nothing prepared: the trace kernel starts them
        GenArgs& gen = nw.gen;
        gen.F = F;
        gen.q_free = q_free; gen.n_gen = (uint32_t)std::min<unsigned long long>(n_free, sample_end - next_sample); gen.n_pix = n_pix; gen.id_base = next_sample;
        gen.sample_begin = sample0; gen.s_begin = s0; gen.pixtab = pixtab; gen.inv_n_pix = 1.0 / (double)n_pix;
        next_sample += gen.n_gen;
        nw.exhausted = next_sample >= sample_end;
        return nw;
    }
};
// a round (run_rounds): the paths k_ad_gen left in work.q_new, all in the first pass; rounds never hand a freed slot out again
struct RoundRefill final : Refill {
    const Frame& F;
    uint32_t pending;
    RoundRefill(const Frame& F_, uint32_t pending_) : F(F_), pending(pending_) {}
    NewPaths next(uint32_t, const uint32_t*) override
    {
        NewPaths nw;
        memset(&nw, 0, sizeof nw);
        nw.gen.F = F;
        nw.n_prepared = pending;
        nw.exhausted = true;
        pending = 0;
        return nw;
    }
};

// ---- the pass loop: trace -> shade -> (keys, sort, gather) -> sort of the continuing rays, until nothing is in flight.  A finished path leaves
// its radiance at lbuf[sample_of(slot) - sample0]: slot_sample is the table the kernels keep that in, or nullptr when the caller knows that slot
// s carries sample sample0 + s throughout.
struct Passes {
    // the call
    gi_ctx* c;
    const Frame& F;
    unsigned long long* slot_sample;
    unsigned long long sample0;
    double* lbuf;
    int& launches;
    bool debug_wf;
    // fixed for the call (passes_begin)
    const StreamGrids* G;
    bool wide, counting;
    int feat, trace_feat;
    uint32_t early_turns, wave_factor;
    PathPool pool;
    StreamCounters* sc;
    ShadowQ* shq;
    // the pass under way
    NewPaths nw;
    uint32_t n_new;                        // prepared + started by the trace kernel
    uint32_t n_cont, n_free, n_gather;     // before the shade stage's read-back: of the pass before
    int ping;
    const uint32_t* free_in;               // the list the pass before wrote (nullptr: none, or slots in order)
    const uint32_t* cont_in;
    uint32_t* cont_out;
    bool want_free;
    uint32_t* free_out;                    // nullptr: nobody will read the list of this pass
    const uint32_t* shade_queue;           // the shade stage's input: work.q_shade, or work.shade_sorted with work.shade_places
    const uint32_t* shade_places;
};

static int passes_begin(Passes& p)
{
    gi_ctx* c = p.c;
    const Frame& F = p.F;
    // the finisher's one-path-per-wave form: up to 2 paths per resident wave (more of them side by side are faster in groups of 16: benchmark frame's
    // finisher 19.6 ms against 27.3 with 32 per wave; closed box 4.4 against 7.0) -- except for a small frame that gathers photons, such as a rank's share
    // of the benchmark frame on 8 GPUs (66 M samples): its tail is a larger part of it and holds fewer paths, and a lone path's gather is the wave
    // routine's: up to 32 (a 1/8 share 60.6 ms against 64.0; tools/fin_share.sh)
    const bool small_frame = (unsigned long long)F.w * (unsigned long long)F.local_rows * (unsigned long long)std::max(F.max_samples, 1) < 200000000ull;
    p.wave_factor = c->tune.wave_factor ? c->tune.wave_factor : ((small_frame && c->S.pcand) ? 32u : 2u);
    p.G = &stream_grids(c);
    if (p.G->lds_refused) return fail(c, GI_E_HIP, "render: the device refused " + std::to_string(p.G->lds_refused) + " bytes of dynamic LDS per workgroup (the traversal kernels are laid out for gfx950's 160 KB per CU)");
    p.wide = c->S.wnodes != nullptr;
    p.feat = scene_feat(c->S); p.trace_feat = scene_trace_feat(c->S);
    // executed-work counters: compiled for the instances the BASELINE scenes run (triangles only, no medium, no texture, shadow walks put off)
    p.counting = c->count_stream;
    if (p.counting && !(p.wide && defers_shadows(c) && !c->S.has_spheres && c->S.n_fog == 0 && c->S.n_tex == 0))
        return fail(c, GI_E_STATE, "render: the streaming work counters (gi_set_counters 2) cover triangle scenes without spheres, fog or textures, walked over wide records with one to four lights; use mode 1 (reference visits, megakernel) for this scene");
    // The probe of the next ray in the deferred shade kernel (ray_leaves_scene): a ray that leaves the scene ends its path there.  Only where such a
    // miss adds nothing and the trace stage's walk culls by content (no ambient light, no medium, content boxes installed, one light: the kernel instance that has the registers for it), and not in a counted
    // frame (its trace_rays are compared with culling on and off).  With it a path that does not continue is released by the shade stage even
    // with a gather pending (k_st_shade).
    const bool no_ambient = c->S.ambient[0] == 0.0 && c->S.ambient[1] == 0.0 && c->S.ambient[2] == 0.0;
    p.early_turns = (c->tune.early_miss && p.wide && defers_shadows(c) && c->S.n_light == 1 && c->S.cboxes != nullptr && c->S.n_fog == 0 && no_ambient && !p.counting) ? c->tune.early_turns : 0u;
    p.pool = make_path_pool(c->st.d_spool.p, c->st.spool_slots);
    p.sc = p.counting ? c->st.d_stream_cnt.p : nullptr;
    p.shq = defers_shadows(c) ? c->st.d_shq.p : nullptr;
    return GI_OK;
}

// a sort of n pairs inside a timed stage, through the workspace's scratch (n keys, then n values), counted as one launch; n_dev as rs_sort_pairs takes it
static int sort_pairs(TimedStage& stage, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, const uint32_t* n_dev, int begin_bit, int end_bit)
{
    gi_ctx* c = stage.c;
    uint32_t* const tk = c->st.work.sort_scratch.p;
    stage.launches++;
    return rs_sort_pairs(c, keys_in, keys_out, vals_in, vals_out, tk, tk + n, n, n_dev, begin_bit, end_bit, c->st.d_rs_hist.p);
}

// The jobs of the two compactions of a pass.  Behind the trace stage: hits -> the shade queue, finished paths -> the head of the free list.
static CompactJob trace_compact_job(const Passes& p)
{
    const StreamWork& w = p.c->st.work;
    CompactJob job;
    memset(&job, 0, sizeof job);
    job.st[0] = {w.stage_hits.p, w.q_shade.p, 1}; job.n_streams[0] = 1; job.kind[0] = QC_SHADE; job.total_field[0] = 0;
    job.st[1] = {w.stage_free_trace.p, p.free_out, 1}; job.n_streams[1] = 1; job.kind[1] = p.want_free ? QC_FREE : -1; job.total_field[1] = 4;
    job.kind[2] = -1; job.gather_queue = -1;
    return job;
}
// Behind the shade stage, streams in queue order: [0] continuing slot, [1] its coherence key, [2] gather slot, [3] gather position (3 doubles = 6 words), [4] freed slot
static CompactJob shade_compact_job(const Passes& p)
{
    const StreamWork& w = p.c->st.work;
    const Scene& S = p.c->S;
    CompactJob job;
    memset(&job, 0, sizeof job);
    job.st[0] = {w.stage_cont_slots.p, w.cont_slots.p, 1}; job.st[1] = {w.stage_cont_keys.p, w.cont_keys.p, 1};
    job.n_streams[0] = 2; job.kind[0] = QC_CONT; job.total_field[0] = 1;
    job.st[2] = {w.stage_gather_slots.p, w.gather_slots.p, 1};      // gather: slot -> values of the sort by leaf
    job.st[3] = {w.stage_gather_pos.p, w.gather_keys.p, 6};         //         position -> key (leaf)
    job.n_streams[1] = 2; job.kind[1] = QC_GATHER; job.total_field[1] = 2; job.gather_queue = S.n_pnode > 0 ? 1 : -1;
    if (S.n_pnode <= 0) job.kind[1] = -1;                           // no photon map: no gather queries
    job.st[4] = {w.stage_free_shade.p, p.free_out, 1};
    job.n_streams[2] = 1; job.kind[2] = p.want_free ? QC_FREE : -1; job.total_field[2] = 3; job.free_base_from_trace = 1;
    return job;
}
static int clear_block_counters(gi_ctx* c)   // the producers' per-workgroup append counters, before each of the two producing kernels
{
    HIP_TRY(c, hipMemsetAsync(c->st.d_blkcnt.p, 0, (size_t)QC_KINDS * GI_MAX_PRODUCER_BLOCKS * GI_CNT_STRIDE * sizeof(unsigned int), c->stream));
    return GI_OK;
}

// The refill has started its last sample, this pass has none to start and few paths are left: the finisher runs them to their ends, stage by
// stage of the plan, the survivors of a stage being the input of the next (both queues are this chunk's continuation queues).
static int finish_tail(Passes& p)
{
    gi_ctx* c = p.c;
    if (c->st.d_fin_cnt.n < 16) HIP_TRY(c, c->st.d_fin_cnt.alloc(16));
    HIP_TRY(c, hipMemsetAsync(c->st.d_fin_cnt.p, 0, 16 * sizeof(unsigned int), c->stream));
    const uint32_t* fq_in = p.cont_in;
    uint32_t* fq_out = p.cont_out;
    const size_t n_stage = std::min<size_t>(c->tune.finish_plan.size(), 15);
    for (size_t k = 0; k < n_stage; k++) {
        const int lanes = c->tune.finish_plan[k].first, vertices = k + 1 == n_stage ? GI_MAX_DEPTH + 1 : c->tune.finish_plan[k].second;
        const unsigned int* n_in_dev = k == 0 ? nullptr : c->st.d_fin_cnt.p + (k - 1);
        TimedStage stage(c, STG_FINISH, p.launches);
        for (int mode = 0; mode < ((p.wide && lanes <= 0) ? 3 : 1); mode++) {   // a path per lane; then, of what that left, a path per wave and a path per group of 16 lanes
            const FinishK fin_k = st_finish(p.feat, p.wide, mode);
            stage.launch(fin_k.fn, dim3(p.G->finish), dim3(GI_FINISH_BLOCK), fin_k.lds, c->S, p.F.seed, p.pool, p.slot_sample, p.sample0,
                         fq_in, n_in_dev, p.n_cont, lanes, vertices, fq_out, c->st.d_fin_cnt.p + k, p.lbuf, (p.wave_factor << 16) | (c->tune.coop_factor & 0xffffu));
        }
        uint32_t* t = const_cast<uint32_t*>(fq_in); fq_in = fq_out; fq_out = t;
    }
    return GI_OK;
}

// trace: new and continuing rays; hits -> staging, finished paths -> staging; compacted into the shade queue and the head of the free list
static int trace_stage(Passes& p)
{
    gi_ctx* c = p.c;
    const StreamWork& w = c->st.work;
    const StreamGrids& G = *p.G;
    HIP_TRY(c, hipMemsetAsync(c->st.d_ctl.p, 0, sizeof(StreamCtl), c->stream));
    // The free list of this pass has one reader, the refill of the next.  Once the refill has started its last sample (`exhausted`, told with the
    // paths of this pass: this pass still reads the previous list, nobody reads the one it would write; rounds never hand a freed slot out again) the
    // kernels get no free queue and skip its appends, the compaction leaves the queue out, and n_free stays 0.  GI_KEEP_FREE_LIST=1: written always.
    p.want_free = c->tune.keep_free_list || !p.nw.exhausted;
    p.free_out = p.want_free ? (p.ping ? w.q_free_b.p : w.q_free_a.p) : nullptr;
    if (G.trace > GI_MAX_PRODUCER_BLOCKS || G.shade > GI_MAX_PRODUCER_BLOCKS) return fail(c, GI_E_STATE, "render: more producer workgroups than per-workgroup counters");
    if (const int rc = clear_block_counters(c)) return rc;
    const TraceK trace_k = st_trace(p.trace_feat, p.wide, p.counting, c->S.lens_radius > 0);
    TimedStage(c, STG_TRACE, p.launches).launch(trace_k.fn, dim3(G.trace), dim3(GI_TRACE_BLOCK), trace_k.lds, c->S, p.F.seed, p.pool, p.slot_sample, p.sample0, p.nw.gen, w.q_new.p, p.nw.n_prepared,
                                                p.cont_in, p.n_cont, c->st.d_blkcnt.p, c->st.d_segs.p, w.stage_hits.p, p.want_free ? w.stage_free_trace.p : nullptr, p.lbuf, c->tune.refill_min, p.sc);
    TimedStage(c, STG_OTHER, p.launches).launch(k_st_compact, dim3(G.compact), dim3(256), 0, c->S, trace_compact_job(p), c->st.d_blkcnt.p, c->st.d_segs.p, (uint32_t)G.trace, c->st.d_ctl.p);
    return GI_OK;
}

// A pass of continuing rays leaves the trace stage in the rays' coherence order, which scatters the shade stage's reads and writes of
// the path records over the whole pool.  The shade queue is put into slot order for it (a radix sort of slot / place pairs); the shadow
// queries still land at the place the trace stage gave the item, so the shadow walks keep that (coherent) order.
static int shade_sort_stage(Passes& p)
{
    gi_ctx* c = p.c;
    const StreamWork& w = c->st.work;
    p.shade_queue = w.q_shade.p;
    p.shade_places = nullptr;
    if (!(c->tune.sort_shade && p.n_cont > 0)) return GI_OK;
    int sbits = 1;
    while ((1ull << sbits) < (unsigned long long)c->st.spool_slots) sbits++;
    const uint32_t bound = p.n_new + p.n_cont;      // every item of the trace stage may have hit something
    int uncounted = 0;                              // n_launches has never included this stage: the figure stays comparable with earlier frames'
    TimedStage stage(c, STG_SORT, uncounted);
    stage.launch(k_iota, dim3(std::min<uint32_t>((bound + 1023u) / 1024u, 4096u)), dim3(1024), 0, w.shade_iota.p, bound);
    if (const int rc = sort_pairs(stage, w.q_shade.p, w.shade_sorted.p, w.shade_iota.p, w.shade_places.p, bound, reinterpret_cast<const uint32_t*>(&c->st.d_ctl.p->n_shade), std::min(c->tune.sort_shade_lo, sbits - 1), sbits)) return rc;
    p.shade_queue = w.shade_sorted.p;
    p.shade_places = w.shade_places.p;
    return GI_OK;
}

// shade: continuing rays (slot + key), gather queries (slot + position) and finished paths -> staging; the shadow walks it put off, before the
// gather of the same vertices (the order in which a path's radiance is summed); the compaction; and the totals of the pass read back
static int shade_stage(Passes& p)
{
    gi_ctx* c = p.c;
    const StreamWork& w = c->st.work;
    const StreamGrids& G = *p.G;
    if (const int rc = clear_block_counters(c)) return rc;
    const bool many = c->S.n_light > 1;
    const ShadeK shade_k = st_shade(p.feat, p.wide, p.shq ? (many ? 2 : 1) : 0);
    TimedStage(c, STG_SHADE, p.launches).launch(shade_k.fn, dim3(G.shade), dim3(GI_SHADE_BLOCK), shade_k.lds, c->S, p.F.seed, p.pool, p.slot_sample, p.sample0, p.shade_queue, c->st.d_ctl.p, c->st.d_blkcnt.p, c->st.d_segs.p,
                                                w.stage_cont_slots.p, w.stage_cont_keys.p, w.stage_gather_slots.p, reinterpret_cast<double*>(w.stage_gather_pos.p), p.want_free ? w.stage_free_shade.p : nullptr,
                                                p.lbuf, p.shq, p.shade_places, p.early_turns);
    if (p.shq) {
        const ShadowK shadow_k = st_shadow(p.feat, many, p.counting);
        TimedStage(c, STG_SHADOW, p.launches).launch(shadow_k.fn, dim3(G.shadow), dim3(GI_SHADOW_BLOCK), shadow_k.lds, c->S, p.F.seed, p.pool, p.shq, c->st.d_ctl.p, p.lbuf, c->tune.refill_min, p.sc);
    }
    TimedStage(c, STG_OTHER, p.launches).launch(k_st_compact, dim3(G.compact), dim3(256), 0, c->S, shade_compact_job(p), c->st.d_blkcnt.p, c->st.d_segs.p, (uint32_t)G.shade, c->st.d_ctl.p);
    HIP_TRY(c, hipMemcpyAsync(c->st.h_ctl.p, c->st.d_ctl.p, sizeof(StreamCtl), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    p.n_gather = c->st.h_ctl.p->n_gather; p.n_cont = c->st.h_ctl.p->n_cont; p.n_free = c->st.h_ctl.p->n_free;
    if (p.counting) c->stream_shaded += c->st.h_ctl.p->n_shade;
    return GI_OK;
}

// the gather queries of the pass in leaf order, and their gather; few queries: a wave each
static int gather_stage(Passes& p)
{
    gi_ctx* c = p.c;
    const StreamWork& w = c->st.work;
    if (!(c->S.n_pnode > 0 && p.n_gather > 0)) return GI_OK;
    {
        TimedStage stage(c, STG_SORT, p.launches);
        if (const int rc = sort_pairs(stage, w.gather_keys.p, w.gather_keys_sorted.p, w.gather_slots.p, w.gather_slots_sorted.p, p.n_gather, nullptr, 0, photon_key_bits(c->S))) return rc;
    }
    TimedStage stage(c, STG_GATHER, p.launches);
    launch_gather(c, c->S.pcand && p.n_gather < c->tune.gather_wave_below, p.counting, p.pool, w.gather_keys_sorted.p, w.gather_slots_sorted.p, p.n_gather, p.slot_sample, p.sample0, p.lbuf, p.sc);
    p.launches++;
    return GI_OK;
}

// continuing rays in coherence order for the next trace pass
static int cont_sort_stage(Passes& p)
{
    gi_ctx* c = p.c;
    const StreamWork& w = c->st.work;
    if (p.n_cont == 0) return GI_OK;
    TimedStage stage(c, STG_SORT, p.launches);
    if (c->tune.sort_cont) {
        return sort_pairs(stage, w.cont_keys.p, w.cont_keys_sorted.p, w.cont_slots.p, p.cont_out, p.n_cont, nullptr, c->tune.sort_lo_bit, 27);
    }
    HIP_TRY(c, hipMemcpyAsync(p.cont_out, w.cont_slots.p, (size_t)p.n_cont * 4, hipMemcpyDeviceToDevice, c->stream));   // GI_SORT_CONT=0: queue order (tuning aid), counted like the sort
    p.launches++;
    return GI_OK;
}

// GI_DEBUG_WF in the environment: a line per pass on stderr.  Read at every call and never kept: the tests set it for single frames.
static bool debug_wf_on() { return getenv("GI_DEBUG_WF") != nullptr; }
static void print_pass(const Passes& p)   // GI_DEBUG_WF
{
    fprintf(stderr, "[st] new %u cont %u free %u gather %u\n", p.n_new, p.n_cont, p.n_free, p.n_gather);
    if (!p.counting) return;
    StreamCounters h;   // what this pass executed (tuning aid): cumulative counters, printed per pass
    if (hipMemcpy(&h, p.c->st.d_stream_cnt.p, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "[cnt] trace rays %llu walks %llu records %llu boxes %llu cboxes %llu leaves %llu eboxes %llu tris %llu | shadow rays %llu records %llu boxes %llu cboxes %llu leaves %llu eboxes %llu tris %llu | gather q %llu cand %llu\n",
                h.trace_rays, h.trace[0], h.trace[1], h.trace[2], h.trace[3], h.trace[4], h.trace[6], h.trace[5], h.shadow_rays, h.shadow[1], h.shadow[2], h.shadow[3], h.shadow[4], h.shadow[6], h.shadow[5], h.gather_queries, h.gather_cand);
}

static int (*const kPassStages[])(Passes&) = {trace_stage, shade_sort_stage, shade_stage, gather_stage, cont_sort_stage};

// n_free: slots free before the first pass (a chunk: the whole pool; a round: none, its paths are prepared); debug_wf: print a line per pass
static int stream_passes(gi_ctx* c, const Frame& F, unsigned long long* slot_sample, unsigned long long sample0, double* lbuf, uint32_t n_free,
                         Refill& refill, bool debug_wf, volatile const int* cancel, int& launches)
{
    Passes p{c, F, slot_sample, sample0, lbuf, launches, debug_wf};
    if (const int rc = passes_begin(p)) return rc;
    p.n_free = n_free;
    for (;;) {
        if (cancel && *cancel) { c->last_launches = launches; return fail(c, GI_E_CANCELLED, "render: cancelled"); }
        p.nw = refill.next(p.n_free, p.free_in);
        p.n_new = p.nw.n_prepared + p.nw.gen.n_gen;
        if (p.n_new + p.n_cont == 0) break;
        p.cont_out = p.ping ? c->st.work.q_cont_b.p : c->st.work.q_cont_a.p;
        p.cont_in = p.ping ? c->st.work.q_cont_a.p : c->st.work.q_cont_b.p;
        if (p.nw.exhausted && p.n_new == 0 && p.n_cont <= c->tune.finish_threshold && !p.counting) return finish_tail(p);   // (a counted frame runs its stragglers through the counting passes)
        for (auto stage : kPassStages)
            if (const int rc = stage(p)) return rc;
        p.free_in = p.free_out;
        p.ping ^= 1;
        if (p.debug_wf) print_pass(p);
    }
    return GI_OK;
}

// Samples [s_begin, s_end) of every pixel of a fixed-spp frame, folded into the records `pix` (st_pixel_xy order) in sample order, one chunk of
// samples at a time; init: the records are put in their initial state first (a frame from sample 0).  The one-shot frame (render_streaming) is
// [0, max_samples) on d_pix with init; a step of a progressive session is [E, E') on the session's records.  s_done (optional) follows the
// samples folded so far, so that a cancelled call tells how far the records got.
static int stream_samples(gi_ctx* c, const Frame& F, PixRec* pix, int s_begin, int s_end, bool init, void* d_out, int out_is_f64, int32_t* d_spp,
                          volatile const int* cancel, int* s_done)
{
    const uint32_t n_pix = (uint32_t)F.w * (uint32_t)F.local_rows;   // valid pixels only, enumerated in 8x8-tile order (st_pixel_xy)
    const int spp = s_end - s_begin;
    const bool debug_wf = debug_wf_on();
    // paths in flight and samples per chunk: gi_layout.h's budget, of free memory plus what this context holds already and would re-use
    size_t free_b = 0, total_b = 0;
    const bool mem_known = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    const PoolPlan plan = plan_pool(mem_known, free_b, c->st.held_bytes(), n_pix, spp, c->tune.pool_slots_max, c->tune.lbuf_bytes_max, defers_shadows(c) ? c->S.n_light : 0);
    const uint32_t P = plan.P;
    const int chunk = plan.chunk;
    // The sample table.  A chunk of ns samples per pixel whose n_pix * ns samples all fit the pool is started whole by the first pass: refill hands
    // the trace stage slots 0 .. n_pix * ns - 1 in order (q_free == nullptr) with sample ids sample0 + slot, and has nothing left to start in a freed slot
    // later.  The table would be the identity plus sample0 for the whole chunk, so the kernels are given none (sample_of) -- 8 bytes per sample less
    // to write in the trace stage and a scattered read less per gather query.  Decided per chunk (fits); the table is allocated when the largest
    // chunk of this call needs it, and stays in the budget per slot either way: a later call may need it.  GI_SAMPLE_IDENTITY=0: always a table.
    auto fits = [&](int ns) { return c->tune.sample_identity && (size_t)P >= (size_t)n_pix * (size_t)ns; };
    int rc = stream_alloc(c, P, !fits(chunk));
    if (rc) return rc;
    if (c->st.d_lbuf.n < (size_t)n_pix * chunk * 3) HIP_TRY(c, c->st.d_lbuf.alloc((size_t)n_pix * chunk * 3));
    const StreamGrids& G = stream_grids(c);
    hipStream_t st = c->stream;
    int launches = 0;
    c->clock.restart();
    if (c->count_stream) {
        if (!c->st.d_stream_cnt.p) HIP_TRY(c, c->st.d_stream_cnt.alloc(1));
        HIP_TRY(c, hipMemsetAsync(c->st.d_stream_cnt.p, 0, sizeof(StreamCounters), st));
        c->stream_shaded = 0;
    }
    HIP_TRY(c, c->t_frame.begin(st));
    if (init) { hipLaunchKernelGGL(k_pix_init, dim3(G.pix), dim3(GI_BLOCK), 0, st, pix, n_pix); launches++; }
    if (c->st.d_pixtab.n < n_pix) HIP_TRY(c, c->st.d_pixtab.alloc(n_pix));
    hipLaunchKernelGGL(k_pixel_table, dim3(G.pix), dim3(GI_BLOCK), 0, st, F, n_pix, c->st.d_pixtab.p);
    launches++;
    for (int s0 = s_begin; s0 < s_end; s0 += chunk) {
        const int ns = std::min(chunk, s_end - s0);
        ChunkRefill refill(F, c->st.d_pixtab.p, n_pix, s0, ns);
        if (debug_wf) fprintf(stderr, "[st] chunk of %d samples: pool %u slots, sample table %s\n", ns, P, fits(ns) ? "off" : "on");
        rc = stream_passes(c, F, fits(ns) ? nullptr : c->st.d_slot_sample.p, refill.sample0, c->st.d_lbuf.p, P, refill, debug_wf, cancel, launches);   // pass 0: every slot is free
        if (rc) return rc;
        TimedStage(c, STG_ACCUM, launches).launch(k_st_accum, dim3(G.accum), dim3(GI_BLOCK), 0, F, pix, c->st.d_lbuf.p, n_pix, ns, d_out, out_is_f64, d_spp);
        if (s_done) *s_done = s0 + ns;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->t_frame.end(st));
    c->last_launches = launches;
    return GI_OK;
}

static int render_streaming(gi_ctx* c, const Frame& F, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    const uint32_t n_pix = (uint32_t)F.w * (uint32_t)F.local_rows;
    if (c->st.d_pix.n < n_pix) HIP_TRY(c, c->st.d_pix.alloc(n_pix));
    return stream_samples(c, F, c->st.d_pix.p, 0, F.max_samples, true, d_out, out_is_f64, d_spp, cancel, nullptr);
}

// Adaptive sampling (min_samples != max_samples, include/raytracer.h:108-148), and every frame of render mode 2: synchronous rounds --
// in a round every pixel that still wants samples starts those it is certain to take (k_ad_gen), the paths run through the streaming
// passes (sorted queues, octree records in LDS, wave-cooperative gather, staged finisher), and k_ad_accum applies the variance rule in
// sample order.  With min_samples == max_samples this renders the fixed-spp frame of render_streaming, a round of up to B samples at a time.
// pix: the records the rounds work on (padded 8x8 tiles); init: put them in their initial state first.  The one-shot frame (render_adaptive) is d_pix
// with init; a step of a progressive session is the session's records with the step's cap E' in F.max_samples -- the same loop, which then stops at E'.
static uint32_t rounds_records(const Frame& F) { return (uint32_t)(((F.w + 7) >> 3) * ((F.local_rows + 7) >> 3)) * 64u; }
static bool rounds_fit(const Frame& F) { return (size_t)((F.w + 7) >> 3) * (size_t)((F.local_rows + 7) >> 3) * 64 <= 0xfffffff0ull; }   // the records, and so a round of them, have 32-bit path slots
static int run_rounds(gi_ctx* c, const Frame& F, PixRec* pix, bool init, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    if (!rounds_fit(F)) return fail(c, GI_E_INVALID, "render: frame too large for 32-bit path slots");
    const uint32_t n_pix = rounds_records(F);   // padded to whole 8x8 tiles (tile_pixel_xy)
    const bool debug_wf = debug_wf_on();
    int B = (int)std::min<size_t>(32, std::max<size_t>(1, std::min<size_t>(c->tune.pool_slots_max, 0xfffffff0ull) / n_pix));
    B = std::max(1, std::min(B, std::max(F.max_samples, 1)));
    const size_t slots = (size_t)n_pix * (size_t)B;
    int rc = stream_alloc(c, (uint32_t)slots, true);   // k_ad_gen names every path's place in the radiance buffer
    if (rc) return rc;
    if (c->st.d_lbuf.n < slots * 3) HIP_TRY(c, c->st.d_lbuf.alloc(slots * 3));
    if (!c->st.d_wfcnt.p) HIP_TRY(c, c->st.d_wfcnt.alloc(2));
    HIP_TRY(c, c->st.h_wfcnt.alloc(2));
    const StreamGrids& G = stream_grids(c);
    hipStream_t st = c->stream;
    unsigned int* cnt = c->st.d_wfcnt.p;
    int launches = 0;
    c->clock.restart();
    HIP_TRY(c, c->t_frame.begin(st));
    if (init) { hipLaunchKernelGGL(k_pix_init, dim3(G.pix), dim3(GI_BLOCK), 0, st, pix, n_pix); launches++; }
    bool any = F.max_samples > 0 && F.min_samples > 0;
    if (!any) {   // 0 samples per pixel still has to write the initial colour
        HIP_TRY(c, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_ad_accum, dim3(G.ad_accum), dim3(GI_BLOCK), 0, st, F, pix, c->st.d_lbuf.p, n_pix, B, d_out, out_is_f64, d_spp, cnt + 1);
        launches++;
    }
    while (any) {
        if (cancel && *cancel) { c->last_launches = launches; return fail(c, GI_E_CANCELLED, "render: cancelled"); }
        HIP_TRY(c, hipMemsetAsync(cnt, 0, 2 * sizeof(unsigned int), st));
        TimedStage(c, STG_REGEN, launches).launch(k_ad_gen, dim3(G.ad_gen), dim3(GI_BLOCK), 0, c->S, F, pix, make_path_pool(c->st.d_spool.p, c->st.spool_slots), c->st.d_slot_sample.p, n_pix, B, c->st.work.q_new.p, cnt + 0);
        HIP_TRY(c, hipMemcpyAsync(c->st.h_wfcnt.p, cnt, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        RoundRefill refill(F, c->st.h_wfcnt.p[0]);      // paths started by this round, already in the new-path queue
        rc = stream_passes(c, F, c->st.d_slot_sample.p, 0ull, c->st.d_lbuf.p, 0u, refill, debug_wf, cancel, launches);
        if (rc) return rc;
        TimedStage(c, STG_ACCUM, launches).launch(k_ad_accum, dim3(G.ad_accum), dim3(GI_BLOCK), 0, F, pix, c->st.d_lbuf.p, n_pix, B, d_out, out_is_f64, d_spp, cnt + 1);
        HIP_TRY(c, hipMemcpyAsync(c->st.h_wfcnt.p + 1, cnt + 1, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        any = c->st.h_wfcnt.p[1] > 0;
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, c->t_frame.end(st));
    c->last_launches = launches;
    return GI_OK;
}

static int render_adaptive(gi_ctx* c, const Frame& F, void* d_out, int out_is_f64, int32_t* d_spp, volatile const int* cancel)
{
    const uint32_t n_pix = rounds_records(F);
    if (c->st.d_pix.n < n_pix) HIP_TRY(c, c->st.d_pix.alloc(n_pix));
    return run_rounds(c, F, c->st.d_pix.p, true, d_out, out_is_f64, d_spp, cancel);
}

// fixed sample count: the streaming pool with path regeneration (the refill schedule); adaptive sampling: rounds (sample-order decisions) on the
// same passes; mode 2: rounds for every frame, a second schedule of the fixed-spp frames
static bool uses_refill_schedule(const gi_ctx* c, const Frame& F) { return c->render_mode == 0 && F.min_samples == F.max_samples && F.max_samples > 0; }

