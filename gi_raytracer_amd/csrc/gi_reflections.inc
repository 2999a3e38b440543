// gi_reflections.inc -- reflection probe sets (gi_render_baked_reflections_*; an addition beside the baked-light pass: box-projected, blended cube
// look-ups for its specular term).  Included by gi_kernels.hip behind gi_baked.inc, whose lit_check and lit_run the entries use and which includes
// the per-lane functions (gi_reflections.h) in front of k_lit.  The definition is stated in include/gi_hip.h.  There is no kernel here: the look-up
// is the RS instances of k_lit (gi_baked.inc, table kLitRs in gi_instances.inc).

namespace {

std::string rs_named(const std::string& err) { return lit_named(err, "render_baked_reflections"); }
// false + message when the set's parameters and pointers are not the header's (behind lit_check, which has seen bp)
bool lit_rs_check(const gi_baked_params* bp, const gi_baked_reflections_params* rp, const void* probes, const void* chains, std::string& err)
{
    if (!rp) { err = "render_baked_reflections: null reflections parameters"; return false; }
    if (rp->n_probes < 0 || rp->n_probes > GI_REFLECTIONS_MAX_PROBES) {
        err = "render_baked_reflections: n_probes must be 0 .. " + std::to_string(GI_REFLECTIONS_MAX_PROBES) + ", got " + std::to_string(rp->n_probes);
        return false;
    }
    if (rp->n_probes > 0 && (bp->terms & GI_BAKED_SPECULAR) && (!probes || !chains)) { err = "render_baked_reflections: the specular term of a probe set needs probes and chains"; return false; }
    return true;
}
// a set with probes and the specular term: the look-up takes part; else the pass is gi_render_baked_*'s, bit for bit
bool lit_rs_active(const gi_baked_params* bp, const gi_baked_reflections_params* rp) { return rp->n_probes > 0 && (bp->terms & GI_BAKED_SPECULAR); }
// lit_check's view of the one chain: not asked for when the set serves the specular term (lit_check asks only whether it is null)
const void* rs_chain_seen(const gi_baked_params* bp, const gi_baked_reflections_params* rp, const void* chain)
{
    return (bp && rp && rp->n_probes > 0 && !chain) ? (const void*)bp : chain;
}
// the host entry looks at the table: every number finite, a box with room on every axis, no negative fade
bool rs_table_ok(const double* probes, int32_t K, std::string& err)
{
    for (int32_t k = 0; k < K; k++) {
        const double* pr = probes + (size_t)k * GI_RS_ROW;
        for (int j = 0; j < GI_RS_ROW; j++)
            if (!std::isfinite(pr[j])) { err = "render_baked_reflections: probe " + std::to_string(k) + " has a non-finite position, box or fade"; return false; }
        for (int a = 0; a < 3; a++)
            if (!(pr[6 + a] > pr[3 + a])) { err = "render_baked_reflections: probe " + std::to_string(k) + " needs box_max > box_min on every axis"; return false; }
        if (pr[9] < 0.0) { err = "render_baked_reflections: probe " + std::to_string(k) + " has a negative fade"; return false; }
    }
    return true;
}

}  // namespace

extern "C" {

void gi_baked_reflections_default_params(gi_baked_reflections_params* p)
{
    if (!p) return;
    p->n_probes = 0;
}

int gi_render_baked_reflections_device(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_reflections_params* rp, const double* d_sh, const double* d_chain,
                                       const double* d_probes, const double* d_chains, void* d_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !d_out) return fail(c, GI_E_INVALID, "render_baked_reflections: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, d_sh, rs_chain_seen(bp, rp, d_chain), err)) return fail(c, GI_E_INVALID, rs_named(err));
    if (!lit_rs_check(bp, rp, d_probes, d_chains, err)) return fail(c, GI_E_INVALID, err);
    Frame F;
    if (const int rc = pixel_pass_frame(c, "render_baked_reflections", p, F)) return rc;
    if (!lit_rs_active(bp, rp))      // no probe takes part: the RS = 0 instances, gi_render_baked_*'s bits
        return lit_run(c, "render_baked_reflections", F, bp, bp->terms, d_sh, d_chain, nullptr, d_out, out_is_f64);
    HIP_TRY(c, hipSetDevice(c->device));
    LitPass& lit = c->lit;
    if (lit.lds_refused < 0) { lit.lds_refused = 0; ask_for_lds(kLit, lit.lds_refused); }       // (pixel_pass would take the RS table's answer for this one)
    if (lit.rs_lds_refused < 0) { lit.rs_lds_refused = 0; ask_for_lds(kLitRs, lit.rs_lds_refused); }
    if (lit.rs_lds_refused) return fail(c, GI_E_HIP, "render_baked_reflections: the device refused " + std::to_string(lit.rs_lds_refused) + " bytes of dynamic LDS per workgroup");
    LitArgs rs{};
    rs.rs_probes = d_probes; rs.rs_chains = d_chains; rs.rs_n = rp->n_probes;
    rs.rs_texels = (uint32_t)cm_texels_before(bp->face, bp->levels);
    return lit_run(c, "render_baked_reflections", F, bp, bp->terms, d_sh, nullptr, &rs, d_out, out_is_f64);
}

int gi_render_baked_reflections_host(gi_ctx* c, const gi_render_params* p, const gi_baked_params* bp, const gi_baked_reflections_params* rp, const double* sh, const double* chain,
                                     const double* probes, const double* chains, void* h_out, int out_is_f64)
{
    if (!c) return GI_E_INVALID;
    if (!p || !h_out) return fail(c, GI_E_INVALID, "render_baked_reflections: null frame parameters or output pointer");
    std::string err;
    if (!lit_check(bp, sh, rs_chain_seen(bp, rp, chain), err)) return fail(c, GI_E_INVALID, rs_named(err));
    if (!lit_rs_check(bp, rp, probes, chains, err)) return fail(c, GI_E_INVALID, err);
    const bool active = lit_rs_active(bp, rp);
    if (active && !rs_table_ok(probes, rp->n_probes, err)) return fail(c, GI_E_INVALID, err);
    if (!c->scene.have_scene) return fail(c, GI_E_STATE, "render_baked_reflections: no scene uploaded");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<double> d_sh, d_chain, d_probes, d_chains;
    if (bp->terms & GI_BAKED_DIFFUSE) HIP_TRY(c, d_sh.upload(sh, (size_t)bp->nx * (size_t)bp->ny * (size_t)bp->nz * 27));
    if (active) {
        HIP_TRY(c, d_probes.upload(probes, (size_t)rp->n_probes * GI_RS_ROW));
        HIP_TRY(c, d_chains.upload(chains, (size_t)rp->n_probes * cm_texels_before(bp->face, bp->levels) * 3));
    } else if (bp->terms & GI_BAKED_SPECULAR)
        HIP_TRY(c, d_chain.upload(chain, cm_texels_before(bp->face, bp->levels) * 3));
    return pixel_pass_to_host(c, c->lit, "render_baked_reflections_host", p, 12, h_out, out_is_f64, nullptr, [&](void* d_out, int32_t*) {
        return gi_render_baked_reflections_device(c, p, bp, rp, d_sh.p, d_chain.p, d_probes.p, d_chains.p, d_out, out_is_f64);
    });
}

}  // extern "C"
