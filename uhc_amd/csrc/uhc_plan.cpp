// uhc_plan.cpp -- batch planning: everything uhc_batch_create decides from the model description, the controller and the UHC_* knobs before it
// allocates anything.  No hip* call in this file; every refusal that does not need the device happens here.
#include "uhc_plan.h"
#include "uhc_delassus_tiles.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static int refuse(std::string* err, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
    return 1;
}

BatchKnobs read_knobs() {
    BatchKnobs k;
    auto is = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
    auto at_least = [](const char* name, int lo, int* v) { if (const char* e = getenv(name)) *v = std::max(lo, atoi(e)); };
    // Guard words (debug): with UHC_GUARD_LDS=1 every region carved below is followed by two doubles nobody owns.  A library built
    // with -DUHC_GUARD_LDS (tools/poison_build.py) fills them with the poison pattern -- the persistent regions' once per env, the constraint
    // phase's after the dynamics temporaries that overlay them are dead -- and reports any that changed (KernelArgs::guard_hits).  The regions
    // move by a few doubles; capacities and tiers stay as they are.  MPR's vertex staging, which runs across three regions on purpose, is off.
    k.guard = is("UHC_GUARD_LDS", '2') ? 2 : is("UHC_GUARD_LDS", '1') ? 1 : 0;  // (2: one "guard" sits ON qpos of the fast tier -- the report must fire: tests/test_gpu_poison.py)
    if (const char* dbg = getenv("UHC_DEBUG")) k.dbg = atoi(dbg);
    if (k.guard) k.dbg |= UHC_DEBUG_NO_VSTAGE;
#ifndef UHC_EXPERIMENTS
    k.dbg &= ~UHC_DEBUG_EXP_MASK;  // (working-set fill, consumer cap, sticky tier 4: measurement switches of tools/ builds: the shipped library does not read them)
#endif
    if (const char* m = getenv("UHC_TIER_MARKS")) sscanf(m, "%d,%d,%d,%d,%d,%d,%d,%d", k.marks + UHC_MARK_UP2_ROWS, k.marks + UHC_MARK_UP2_CON, k.marks + UHC_MARK_UP2_TWO, k.marks + UHC_MARK_DN1_ROWS, k.marks + UHC_MARK_DN1_CON, k.marks + UHC_MARK_DN1_TWO, k.marks + UHC_MARK_UP3_8THS, k.marks + UHC_MARK_DN2_8THS);
    // UHC_FAST_DENSE = "KiB,dense rows[,contacts]": the dense fast tier's LDS budget, body-body row slots and contact capacity (experiments)
    if (const char* fd = getenv("UHC_FAST_DENSE")) k.fast_dense_got = sscanf(fd, "%d,%d,%d", &k.fast_dense_kib, &k.fast_dense_rows, &k.fast_dense_con);
    k.fast_dcol_own = is("UHC_FAST_DCOL_OWN", '1');
    // occupancy experiments (tools/occupancy_sweep.sh): UHC_LDS_PAD_FAST = KiB the fast tier's launch ASKS for -- the layout
    // is unchanged, the workgroup merely occupies more of the CU's 160 KiB, so fewer of them share a CU (64: two, 100: one)
    if (const char* pad = getenv("UHC_LDS_PAD_FAST")) { k.lds_pad_fast = true; k.lds_pad_fast_kib = atoi(pad); }
    k.force_general = is("UHC_FORCE_GENERAL", '1');
    k.tiers = is("UHC_TIERS", '2') ? 2 : is("UHC_TIERS", '3') ? 3 : 0;
    at_least("UHC_Q2_DIV", 1, &k.q2_div); at_least("UHC_Q2_WAIT", 1, &k.q2_wait_min); at_least("UHC_Q2_MAX", 16, &k.q2_max);
    at_least("UHC_Q3_MAX", 2, &k.q3_max); at_least("UHC_Q4_MAX", 0, &k.q4_max); at_least("UHC_T4_ROWS", 0, &k.t4_rows);
    if (const char* fc = getenv("UHC_FAST_CHUNK")) {  // (strict: a typo must not silently select the default)
        char* end = nullptr;
        const long v = strtol(fc, &end, 10);
        if (end == fc || *end != 0 || v < 0) k.fast_chunk_bad = true;
        else k.fast_chunk = (v == 0 || v > 0x7fff) ? 0x7fff : (int)v;
    }
    return k;
}

static bool same_topology(const UhcModelDesc& a, const UhcModelDesc& b) {
    if (a.nq != b.nq || a.nv != b.nv || a.nu != b.nu || a.nbody != b.nbody || a.njnt != b.njnt || a.ngeom != b.ngeom ||
        a.nmeshvert != b.nmeshvert || a.nexclude != b.nexclude)  // (hull graphs may differ: they live in the model blobs)
        return false;
    auto eq = [](const int32_t* x, const int32_t* y, size_t n) { return !memcmp(x, y, n * 4); };
    return eq(a.body_parentid, b.body_parentid, a.nbody) && eq(a.jnt_type, b.jnt_type, a.njnt) &&
           eq(a.jnt_bodyid, b.jnt_bodyid, a.njnt) && eq(a.dof_parentid, b.dof_parentid, a.nv) &&
           eq(a.geom_type, b.geom_type, a.ngeom) && eq(a.geom_bodyid, b.geom_bodyid, a.ngeom) &&
           eq(a.geom_vertadr, b.geom_vertadr, a.ngeom) && eq(a.geom_vertnum, b.geom_vertnum, a.ngeom) &&
           eq(a.geom_contype, b.geom_contype, a.ngeom) && eq(a.geom_conaffinity, b.geom_conaffinity, a.ngeom) &&
           eq(a.jnt_limited, b.jnt_limited, a.njnt) && eq(a.geom_condim, b.geom_condim, a.ngeom);
}

static void build_blob(const UhcModelDesc& d, DevNumOff& o, std::vector<double>& blob, int adjdeg) {
    blob.clear();
    auto put = [&](const double* p, size_t n) { int off = (int)blob.size(); blob.insert(blob.end(), p, p + n); return off; };
    o.body_pos = put(d.body_pos, 3 * d.nbody); o.body_quat = put(d.body_quat, 4 * d.nbody);
    o.body_ipos = put(d.body_ipos, 3 * d.nbody); o.body_iquat = put(d.body_iquat, 4 * d.nbody);
    o.body_mass = put(d.body_mass, d.nbody); o.body_inertia = put(d.body_inertia, 3 * d.nbody);
    o.body_invweight0 = put(d.body_invweight0, 2 * d.nbody);
    o.jnt_pos = put(d.jnt_pos, 3 * d.njnt); o.jnt_axis = put(d.jnt_axis, 3 * d.njnt); o.jnt_range = put(d.jnt_range, 2 * d.njnt);
    o.jnt_stiffness = put(d.jnt_stiffness, d.njnt); o.jnt_margin = put(d.jnt_margin, d.njnt);
    o.qpos0 = put(d.qpos0, d.nq); o.qpos_spring = put(d.qpos_spring, d.nq);
    o.dof_armature = put(d.dof_armature, d.nv); o.dof_damping = put(d.dof_damping, d.nv);
    o.dof_frictionloss = put(d.dof_frictionloss, d.nv); o.dof_invweight0 = put(d.dof_invweight0, d.nv);
    o.geom_pos = put(d.geom_pos, 3 * d.ngeom); o.geom_quat = put(d.geom_quat, 4 * d.ngeom);
    o.geom_friction = put(d.geom_friction, 3 * d.ngeom); o.geom_margin = put(d.geom_margin, d.ngeom);
    o.geom_gap = put(d.geom_gap, d.ngeom); o.geom_solref = put(d.geom_solref, 2 * d.ngeom);
    o.geom_solimp = put(d.geom_solimp, 5 * d.ngeom); o.geom_rbound = put(d.geom_rbound, d.ngeom);
    o.geom_center = put(d.geom_center, 3 * d.ngeom);
    o.mesh_vert = put(d.mesh_vert, 3 * (size_t)d.nmeshvert);
    {   // box around every hull in its body's frame (centre, half extents): the second cull of the convex pairs (after the bounding spheres)
        std::vector<double> box((size_t)6 * std::max(d.ngeom, 1), 0.0);
        for (int g = 0; g < d.ngeom; g++) {
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            const int v0 = d.geom_vertadr ? d.geom_vertadr[g] : 0, nvt = d.geom_vertnum ? d.geom_vertnum[g] : 0;
            for (int v = v0; v < v0 + nvt; v++)
                for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], d.mesh_vert[3 * v + k]); hi[k] = std::max(hi[k], d.mesh_vert[3 * v + k]); }
            const double rr = (d.geom_type[g] == UHC_GEOM_SPHERE || d.geom_type[g] == UHC_GEOM_CAPSULE) ? d.geom_size[3 * g] : 0.0;  // a rounded hull reaches its radius beyond the core
            for (int k = 0; k < 3; k++) {
                if (nvt > 0) { box[6 * g + k] = 0.5 * (lo[k] + hi[k]); box[6 * g + 3 + k] = 0.5 * (hi[k] - lo[k]) + rr; }
                else { box[6 * g + k] = d.geom_center[3 * g + k]; box[6 * g + 3 + k] = d.geom_rbound[g]; }  // (no hull: the bounding sphere's box)
            }
        }
        o.geom_box = put(box.data(), box.size());
        std::vector<double> rad((size_t)std::max(d.ngeom, 1), 0.0);
        for (int g = 0; g < d.ngeom; g++)
            if (d.geom_type[g] == UHC_GEOM_SPHERE || d.geom_type[g] == UHC_GEOM_CAPSULE) rad[g] = d.geom_size[3 * g];
        o.geom_radius = put(rad.data(), rad.size());
    }
    o.actuator_gear = put(d.actuator_gear, 3 * (size_t)d.nu);
    o.meaninertia = put(&d.meaninertia, 1);
    {   // hull graph: fixed stride, neighbour order = the CSR's order (the multi-contact rule takes neighbours in that order)
        std::vector<int32_t> adj((size_t)std::max(d.nmeshvert, 1) * adjdeg + 2, -1);
        for (int v = 0; v < d.nmeshvert; v++)
            for (int e = d.mesh_adjadr[v], k = 0; e < d.mesh_adjadr[v + 1]; e++, k++) adj[(size_t)v * adjdeg + k] = d.mesh_adj[e];
        std::vector<double> packed((adj.size() + 1) / 2, 0.0);
        memcpy(packed.data(), adj.data(), adj.size() / 2 * 2 * sizeof(int32_t));
        o.mesh_adj = put(packed.data(), packed.size());
    }
    while (blob.size() % 2) blob.push_back(0.0);
    o.stride = (int)blob.size();
}

// ------------------------------------------------------------------ validation
static int validate(const UhcModel* const* models, int n_models, const int32_t* env_model, int n_env, const UhcCtrlDesc* ctrl, int* n_trail_out, std::string* err) {
    if (!models || n_models < 1 || n_env < 1 || !ctrl) return refuse(err, "uhc_batch_create: bad argument");
    const UhcModelDesc& d = models[0]->d;
    for (int k = 1; k < n_models; k++)
        if (!same_topology(d, models[k]->d)) return refuse(err, "uhc_batch_create: model %d differs in topology from model 0", k);
    if (env_model)
        for (int e = 0; e < n_env; e++)
            if (env_model[e] < 0 || env_model[e] >= n_models) return refuse(err, "uhc_batch_create: env_model[%d] out of range", e);
    // free bodies at the end of the model (objects: a body under the world with one free joint and no children, after the humanoid)
    int n_trail = 0;
    for (int j = d.njnt - 1; j >= 1 && d.jnt_type[j] == UHC_JNT_FREE && d.body_parentid[d.jnt_bodyid[j]] == 0 && d.jnt_bodyid[j] == d.nbody - 1 - n_trail; j--) n_trail++;
    // the stable-PD controller works on the humanoid's block of M (the reference cuts M to [:qvel_lim, :qvel_lim], humanoid_im.py:1021-1022;
    // objects are separate trees, so the solve over all dofs gives the same humanoid accelerations)
    if (ctrl->action_type == 0 && d.nq - 7 * n_trail != d.nv - 6 * n_trail + 1) return refuse(err, "uhc_batch_create: PD control expects a free root + scalar joints (+ free objects behind them)");
    if (ctrl->action_type == 0 && d.nu != d.nv - 6 * n_trail - 6) return refuse(err, "uhc_batch_create: PD control expects one motor per non-root dof of the humanoid");
    *n_trail_out = n_trail;
    return 0;
}

// ------------------------------------------------------------------ derived topology tables
static void tree_tables(const UhcModelDesc& d, BatchPlan& P) {
    const int nb = d.nbody, nv = d.nv;
    DevTopo& T = P.A.t;
    P.body_depth.assign(nb, 0); P.body_rootid.assign(nb, 0); P.body_nsub.assign(nb, 1); P.body_lastdof.assign(nb, -1);
    for (int i = 1; i < nb; i++) {
        int p = d.body_parentid[i];
        P.body_depth[i] = P.body_depth[p] + 1;
        P.body_rootid[i] = p == 0 ? i : P.body_rootid[p];
        P.body_lastdof[i] = d.body_dofnum[i] > 0 ? d.body_dofadr[i] + d.body_dofnum[i] - 1 : P.body_lastdof[p];
    }
    for (int i = nb - 1; i > 0; i--) P.body_nsub[d.body_parentid[i]] += P.body_nsub[i];
    T.body_maxdepth = *std::max_element(P.body_depth.begin(), P.body_depth.end());
    P.dof_depth.assign(nv, 0); P.dof_ndesc.assign(nv, 0);
    for (int i = 0; i < nv; i++) P.dof_depth[i] = d.dof_parentid[i] < 0 ? 0 : P.dof_depth[d.dof_parentid[i]] + 1;
    for (int i = nv - 1; i >= 0; i--)
        if (d.dof_parentid[i] >= 0) P.dof_ndesc[d.dof_parentid[i]] += P.dof_ndesc[i] + 1;
    T.maxdepth = *std::max_element(P.dof_depth.begin(), P.dof_depth.end());
    const int YS = T.maxdepth + 1;
    P.dof_anc.assign((size_t)nv * YS, 0); P.m_row.assign(T.nM, 0); P.m_col.assign(T.nM, 0);
    for (int i = 0; i < nv; i++) {
        int k = i;
        for (int q = P.dof_depth[i]; q >= 0; q--) { P.dof_anc[(size_t)i * YS + q] = (short)k; k = d.dof_parentid[k]; }
        int adr = d.dof_madr[i];
        for (int j = i; j >= 0; j = d.dof_parentid[j], adr++) { P.m_row[adr] = (short)i; P.m_col[adr] = (short)j; }
    }
    P.m_ij.assign(T.nM + 4, 0);
    for (int e = 0; e < T.nM; e++) P.m_ij[e] = (unsigned short)((P.m_row[e] << 8) | P.m_col[e]);
    // (host only since the Delassus build reads the chains as masks, below: kept for the plan recording, which hashes it; to retire with the recording)
    P.ncommon.assign((size_t)nv * nv, 0);
    for (int i = 0; i < nv; i++)
        for (int j = 0; j < nv; j++) {
            int q = 0;
            const int lim = std::min(P.dof_depth[i], P.dof_depth[j]);
            while (q <= lim && P.dof_anc[(size_t)i * YS + q] == P.dof_anc[(size_t)j * YS + q]) q++;
            P.ncommon[(size_t)i * nv + j] = (unsigned char)q;
        }
    // the chains as bit masks: the Delassus build finds a dof's position on a chain by counting the chain's dofs below it (uhc_delassus_tiles.h)
    P.chainmask.assign((size_t)nv * 2, 0ull);
    for (int i = 0; i < nv; i++) dt_chain_mask(d.dof_parentid, i, &P.chainmask[(size_t)i * 2], &P.chainmask[(size_t)i * 2 + 1]);
    P.dof_rootid.assign(nv, 0);
    for (int i = 0; i < nv; i++) P.dof_rootid[i] = P.body_rootid[d.dof_bodyid[i]];
}
// what the kernels rely on in the trees
static int validate_trees(const UhcModelDesc& d, const BatchPlan& P, std::string* err) {
    const int nb = d.nbody, nv = d.nv;
    for (int i = 1; i < nb; i++) {  // DFS order check: subtree must be the contiguous range [i, i+nsub)
        for (int c = i + 1; c < i + P.body_nsub[i]; c++) {
            int p = c;
            while (p > i) p = d.body_parentid[p];
            if (p != i) return refuse(err, "uhc_batch_create: bodies are not in depth-first order");
        }
    }
    if (nb > 32) return refuse(err, "uhc_batch_create: %d bodies > 32 (subtree force sums use three 64-lane passes of 6 components)", nb);
    for (int i = 1; i < nb; i++)
        if (d.body_jntnum[i] > 8) return refuse(err, "uhc_batch_create: body %d has %d joints (> 8)", i, d.body_jntnum[i]);
    for (int i = 0; i < nv; i++)
        for (int c = i + 1; c <= i + P.dof_ndesc[i]; c++) {
            int p = c;
            while (p > i) p = d.dof_parentid[p];
            if (p != i) return refuse(err, "uhc_batch_create: dofs are not in depth-first order");
        }
    if (P.A.t.maxdepth + 1 > 32) return refuse(err, "uhc_batch_create: dof chain depth %d > 32 unsupported", P.A.t.maxdepth + 1);
    return 0;
}

// statically filtered collision pairs (plane, mesh)
static int collision_pairs(const UhcModelDesc& d, BatchPlan& P, std::string* err) {
    int skipped_pairs = 0;
    for (int g1 = 0; g1 < d.ngeom; g1++)
        for (int g2 = g1 + 1; g2 < d.ngeom; g2++) {
            int b1 = d.geom_bodyid[g1], b2 = d.geom_bodyid[g2];
            if (!((d.geom_contype[g1] & d.geom_conaffinity[g2]) || (d.geom_contype[g2] & d.geom_conaffinity[g1]))) continue;
            if (b1 == b2) continue;
            if (b1 != 0 && b2 != 0 && (d.body_parentid[b1] == b2 || d.body_parentid[b2] == b1)) continue;
            bool ex = false;
            for (int e = 0; e < d.nexclude; e++) {
                int x = d.exclude_pair[2 * e], y = d.exclude_pair[2 * e + 1];
                if ((x == b1 && y == b2) || (x == b2 && y == b1)) ex = true;
            }
            if (ex) continue;
            int t1 = d.geom_type[g1], t2 = d.geom_type[g2];
            if (P.body_lastdof[b1] < 0 && P.body_lastdof[b2] < 0) continue;  // two static bodies never collide ([MJ-ext] same weld id)
            // hulls: meshes and the rounded hulls (sphere = one core vertex, capsule = two, + a radius: include/uhc_amd.h) -- with vertices in the mesh tables
            auto hull = [&](int g, int t) { return (t == UHC_GEOM_MESH || t == UHC_GEOM_SPHERE || t == UHC_GEOM_CAPSULE) && d.geom_vertnum[g] > 0; };
            if (t1 == UHC_GEOM_PLANE && hull(g2, t2) && b1 == 0) { P.pg1.push_back(g1); P.pg2.push_back(g2); }
            else if (t2 == UHC_GEOM_PLANE && hull(g1, t1) && b2 == 0) { P.pg1.push_back(g2); P.pg2.push_back(g1); }
            else if (hull(g1, t1) && hull(g2, t2)) { P.cg1.push_back(g1); P.cg2.push_back(g2); }
            else skipped_pairs++;
        }
    if (skipped_pairs) return refuse(err, "uhc_batch_create: %d collision pairs of unsupported geom types (built: plane-hull, hull-hull; a hull is a mesh, a sphere or a capsule)", skipped_pairs);
    P.A.t.npair = (int)P.pg1.size();
    P.A.t.ncpair = (int)P.cg1.size();
    return 0;
}

// numeric blobs, one per model
static int model_blobs(const UhcModel* const* models, int n_models, BatchPlan& P, std::string* err) {
    KernelArgs& A = P.A;
    std::vector<double> one;
    A.adjdeg = 1;
    for (int k = 0; k < n_models; k++)
        for (int v = 0; v < models[k]->d.nmeshvert; v++) A.adjdeg = std::max(A.adjdeg, models[k]->d.mesh_adjadr[v + 1] - models[k]->d.mesh_adjadr[v]);
    if (A.adjdeg > UHC_WAVE - 1) return refuse(err, "uhc_batch_create: a hull vertex with %d neighbours (> 63)", A.adjdeg);
    for (int k = 0; k < n_models; k++) {
        build_blob(models[k]->d, A.o, one, A.adjdeg);
        P.model_blob.insert(P.model_blob.end(), one.begin(), one.end());
    }
    return 0;
}

static int controller(const UhcModelDesc& d, const UhcCtrlDesc* ctrl, BatchPlan& P, std::string* err) {
    DevCtrl& C = P.A.c;
    C.n_substeps = ctrl->n_substeps; C.action_type = ctrl->action_type; C.meta_pd = ctrl->meta_pd; C.rfc_mode = ctrl->rfc_mode;
    C.action_dim = ctrl->action_dim; C.rfc_scale = ctrl->rfc_scale; C.rfc_lim = ctrl->rfc_lim;
    {
        const double* q = ctrl->base_rot;
        double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (n2 <= 0) return refuse(err, "uhc_batch_create: zero base_rot");
        C.base_rot_inv[0] = q[0] / n2; C.base_rot_inv[1] = -q[1] / n2; C.base_rot_inv[2] = -q[2] / n2; C.base_rot_inv[3] = -q[3] / n2;
    }
    C.n_vf_body = 0; C.body_vf_dim = 0; C.vf_body = nullptr;
    if (C.rfc_mode == 2) {
        C.n_vf_body = ctrl->n_vf_body; C.body_vf_dim = ctrl->body_vf_dim;
        if (C.n_vf_body < 1 || C.n_vf_body > 64 || !ctrl->vf_body || (C.body_vf_dim != 6 && C.body_vf_dim != 9))
            return refuse(err, "uhc_batch_create: explicit RFC needs 1..64 vf bodies and body_vf_dim 6 or 9");
        P.vf_body.assign(ctrl->vf_body, ctrl->vf_body + C.n_vf_body);
        std::vector<int> seen(d.nbody, 0);
        for (int v : P.vf_body)
            if (v < 0 || v >= d.nbody || seen[v]++) return refuse(err, "uhc_batch_create: vf_body ids must be distinct model bodies");
    } else if (C.rfc_mode != 0 && C.rfc_mode != 1) return refuse(err, "uhc_batch_create: rfc_mode must be 0, 1 or 2");
    const int min_adim = d.nu + (C.rfc_mode == 1 ? 6 : C.rfc_mode == 2 ? C.n_vf_body * C.body_vf_dim : 0) + (C.meta_pd == 1 ? 2 * C.n_substeps : C.meta_pd == 2 ? 2 * d.nu : 0);
    if (C.action_dim < min_adim) return refuse(err, "uhc_batch_create: action_dim %d < %d required by the controller", C.action_dim, min_adim);
    return 0;
}

// ------------------------------------------------------------------ LDS layouts
// LDS carve (doubles; every offset even => 16-byte aligned).  Every tier's layout has a persistent part (state, the factor of M,
// body poses, cdof) and ONE region shared by the dynamics temporaries (first half of a forward pass) and the constraint data
// (second half).  M itself is parked in registers between substeps (MPark), so no tier keeps a second copy in LDS.
struct Carver {
    bool guard_on = false;            // UHC_GUARD_LDS: two doubles nobody owns behind every recorded region
    int off = 0;
    int end1 = 0;                     // where the dynamics temporaries of phase 1 end
    std::vector<int> persist, phase2; // this layout's guard words: after the persistent / the constraint-phase regions
    std::vector<int>* rec = nullptr;  // the list the next carve records its guard in (null: phase 1, overlaid by the constraint data, no guards)
    int carve(int n) { int o = off; off += (n + 1) & ~1; if (guard_on && rec) { rec->push_back(off); off += 2; } return o; }
    void end_guard() { if (guard_on) { phase2.push_back(off); off += 2; } }
};
// persistent part + phase 1; leaves the carver where phase 2 starts (fast: with the (row, col) table of M in LDS)
static void common_layout(Carver& cv, const UhcModelDesc& d, const DevTopo& T, DevLds& F, bool fast) {
    const int nv = d.nv, nb = d.nbody, nj = d.njnt;
    cv.off = 0;
    cv.persist.clear(); cv.phase2.clear(); cv.rec = &cv.persist;
    F.qpos = cv.carve(d.nq); F.qvel = cv.carve(nv); F.qacc = cv.carve(nv); F.ctrl = cv.carve(d.nu); F.applied = cv.carve(nv);
    F.bias = cv.carve(nv); F.smooth = cv.carve(nv); F.z = cv.carve(nv); F.dinv = cv.carve(nv); F.sdinv = cv.carve(nv);
    F.zero = cv.carve(2);
    F.mij = fast ? cv.carve((T.nM + 3) / 4 + 1) : 0;  // the larger tiers read the (row, col) table from L2 and keep the LDS for rows
    F.LD = cv.carve(T.nM + 2); F.M = F.LD;
    F.cdof = cv.carve(6 * nv);
    F.xpos = cv.carve(3 * nb); F.xquat = cv.carve(4 * nb); F.xmat = cv.carve(9 * nb); F.xipos = cv.carve(3 * nb); F.rootcom = cv.carve(3 * nb);
    F.vec = fast ? F.z : cv.carve(nv);  // the working sets accumulate z over islands in vec
    const int base = cv.off;
    cv.rec = nullptr;  // (phase 1: overlaid by the constraint data, no guards)
    // phase 1
    F.cinert = cv.carve(10 * nb);
    const int r2 = cv.off;
    F.ximat = cv.carve(9 * nb); F.xanchor = cv.carve(3 * nj); F.xaxis = cv.carve(3 * nj);  // dead after k_com_pos
    const int endA = cv.off;
    cv.off = r2;
    F.cdofdot = cv.carve(6 * nv);
    const int r3 = cv.off;
    F.crb = cv.carve(10 * nb);                                                        // k_crb only
    const int endB = cv.off;
    cv.off = r3;
    F.cvel = cv.carve(6 * nb); F.cacc = cv.carve(6 * nb); F.cfrc = cv.carve(6 * nb);         // k_com_vel .. k_rne
    cv.end1 = std::max(std::max(endA, endB), cv.off);
    cv.off = base;
    cv.rec = &cv.phase2;
}

// ---- fast tier: target 40 KiB per workgroup => 4 workgroups (one per SIMD) per CU
static void fast_layout(Carver& cv, const UhcModelDesc& d, int n_env, const BatchKnobs& knobs, BatchPlan& P) {
    KernelArgs& A = P.A;
    const DevTopo& T = A.t;
    DevLds& F = A.lf;
    const int YS = T.maxdepth + 1;
    common_layout(cv, d, T, F, T.ncpair == 0);  // (the DENSE instantiations read the (row, col) table of M from L2, like the larger tiers: 2.4 KiB for rows)
    // UHC_FAST_DENSE = "KiB,dense rows[,contacts]": the dense fast tier's LDS budget, body-body row slots and contact capacity (experiments)
    int dense_kib = 52, fast_maxcon = UHC_FAST_MAXCON, fast_ndense = UHC_FAST_MAXTWO;
    if (T.ncpair > 0) fast_maxcon = UHC_FAST_MAXCON_DENSE;
    // A batch of four or more rounds of the 3-per-CU layout (>= 3072 envs on 256 CUs) is throughput-bound by how many fast-tier
    // workgroups a CU holds, not by the general tier's slowest env: it gets the 40 KiB layout with 6 body-body row slots -- 4 per CU, one
    // per SIMD; 12 % of the env-steps go through the general tier instead of 2.6 %.  Measured on the generated model class, env-steps/s
    // with 52 KiB / 12 slots -> 40 KiB / 6 slots: 1024 envs 88 k -> 88 k, 2048 envs 119 k -> 98 k (250 envs per step queue for the general
    // tier's consumers), 3072 envs 112 k -> 141 k, 4096 envs (configs[2]'s share of one GPU) 100 k -> 141 k.
    // Only for a humanoid of hinge joints without objects: a ball-joint humanoid folds into itself and boxes bring 16 rows each, their envs
    // need the 12 slots -- with 6, 95 % of configs[4]'s env-steps at 4096 envs went through the general tier (tier trace
    // r04_v6_tier_trace_configs4_4096.txt), `ball_rollout` took 53 ms per step against 37-43 ms with the wide layout.
    bool hinge_only = P.n_trailing_free == 0;
    for (int j = 0; j < d.njnt; j++) hinge_only = hinge_only && d.jnt_type[j] != UHC_JNT_BALL;
    if (T.ncpair > 0 && n_env >= 3072 && hinge_only) { dense_kib = 40; fast_ndense = 6; }
    // A BALL-JOINT humanoid gets 9 body-body row slots instead of 12 (round 6): three dense rows less are 370 doubles more for the packed rows, whose storage names
    // two of three hand-ons of the ball-joint rollouts (long dof chains, three dofs per joint).  Measured on one box, 3 x 60 steps, env-steps/s with 12 / 9 / 8 / 7 slots:
    // `ball_rollout` 54.1 k / 65.8 k / 65.6 k / 62.4 k, `configs4` 57.3 k / 58.4 k / 57.5 k / 54.5 k (profiles/r06_fd_dense_slots.txt); the hinge models keep 12
    // (headline 96.5 k with 12, 96.4 k with 10, 95.4 k with 8; `shapes` 101.1 / 100.7 / 98.7 k).
    bool any_ball = false;
    for (int j = 0; j < d.njnt; j++) any_ball = any_ball || d.jnt_type[j] == UHC_JNT_BALL;
    if (T.ncpair > 0 && any_ball && dense_kib == 52) fast_ndense = 9;
    {
        const int got = knobs.fast_dense_got, kib = knobs.fast_dense_kib, nd = knobs.fast_dense_rows, nc = knobs.fast_dense_con;
        // (a model with convex pairs keeps at least one body-body slot: the layout drops the (row, col) table of M from LDS for such a model
        //  and the launcher picks the DENSE instantiation -- which reads the table from L2 -- by `cf.ndense > 0`: nd = 0 would launch
        //  <0, 1, false> on a layout without the table it indexes)
        if (got >= 2 && kib >= 32 && kib <= 160 && nd >= (T.ncpair > 0 ? 1 : 0) && nd <= UHC_FAST_MAXTWO) { dense_kib = kib; fast_ndense = nd; }
        if (got == 3 && nc >= 8 && nc <= UHC_GEN_MAXCON && T.ncpair > 0) fast_maxcon = nc;
    }
    F.con = cv.carve(fast_maxcon * UHC_CON_STRIDE);
    F.rowMisc = cv.carve(UHC_WAVE * 2);
    F.ncon_nefc = cv.carve(2 + UHC_MAXTWO / 2);
    // models with body-body contacts (self-collision, objects) keep up to UHC_FAST_MAXTWO dense rows + their Delassus columns; they
    // get a third of the CU's LDS (3 workgroups per CU) instead of a quarter -- the stock floor-only model keeps its 40 KiB layout
    A.cf.maxefc = UHC_FAST_MAXEFC; A.cf.maxcon = fast_maxcon; A.cf.ld_delta = 0;
    A.cf.ndense = T.ncpair > 0 ? fast_ndense : 0;
    F.dense = cv.carve(A.cf.ndense * A.nvp);
    // the dense rows' Delassus columns are written by the contact solve, when nothing reads the contacts any more (the rows are built):
    // they take the contacts' storage when they fit it (6 slots x 64 lanes = 16 contacts x 24 doubles), as in the larger tiers
    const bool dcol_alias = A.cf.ndense * UHC_WAVE <= fast_maxcon * UHC_CON_STRIDE && !knobs.fast_dcol_own;
    // (no kernel writes or reads dcol any more -- the dense rows' entries of A come out of the same tiles as the rest, uhc_delassus_tiles.h -- so UHC_FAST_DCOL_OWN=1 only
    //  spends LDS; offset and knob stay because the recorded layouts of tests/batch_plan_recording.json name them.  To retire together with that recording)
    F.dcol = dcol_alias ? F.con : cv.carve(A.cf.ndense * UHC_WAVE);
    F.Y = cv.off;
    // (52 KiB, not 160 / 3 = 53.3: the LDS is handed out in granules, and 54 608 B rounded up no longer fits three times -- the tier
    //  trace showed 512 of 1 024 workgroups resident, two per CU; 52 KiB is a whole number of every granule up to 4 KiB)
    const int budget = T.ncpair > 0 ? (dense_kib * 1024) / 8 : 40 * 1024 / 8;
    int ycap = budget - cv.off - (cv.guard_on ? 2 : 0);
    const int need1 = cv.end1 - cv.off;  // phase 1 may need more than the constraint data
    if (ycap < need1) ycap = need1;
    if (ycap < 8 * YS) ycap = 8 * YS;
    A.cf.ycap = ycap;
    A.cf.vstage = ((A.dbg & UHC_DEBUG_NO_VSTAGE) == 0 && T.ncpair > 0 && 3 * d.nmeshvert <= A.cf.ndense * A.nvp + (dcol_alias ? 0 : A.cf.ndense * UHC_WAVE) + ycap) ? F.dense : -1;  // dense, (dcol,) Y are contiguous
    cv.off += ycap;
    cv.end_guard();
    F.rowR = F.rowAref = F.rowB = F.rowF = F.rowDa = F.rowW = F.rowY = F.dsc = F.Y;  // unused by the fast kernel
    F.total = cv.off;
    if (A.marks[UHC_MARK_UP2_TWO] < 0) {  // the marks follow the layout: up at the capacity, down with a little room to spare
        A.marks[UHC_MARK_UP2_TWO] = A.cf.ndense > 0 ? A.cf.ndense : UHC_FAST_MAXTWO; A.marks[UHC_MARK_DN1_TWO] = A.cf.ndense > 0 ? std::max(1, A.cf.ndense - (A.cf.ndense > 8 ? 2 : 1)) : 10;
        A.marks[UHC_MARK_UP2_CON] = A.cf.maxcon; A.marks[UHC_MARK_DN1_CON] = A.cf.maxcon - std::max(2, A.cf.maxcon / 8);
    }
    P.lds_bytes_fast = (size_t)cv.off * sizeof(double);
    if (knobs.lds_pad_fast) {  // UHC_LDS_PAD_FAST (read_knobs): the launch asks for more than the layout needs
        const size_t want = (size_t)knobs.lds_pad_fast_kib * 1024;
        if (want > P.lds_bytes_fast && want <= 160 * 1024) P.lds_bytes_fast = want;
    }
    P.use_fast = !knobs.force_general && P.lds_bytes_fast <= 160 * 1024;
}

// ---- general / large tiers: rows two (four) per lane, Yhat packed row after row.  The general tier is sized for TWO workgroups per CU
//      (<= 79 KiB): its Yhat storage is what that budget leaves, and an env whose packed rows (or contacts, rows, dense rows) do not
//      fit goes on to the large tier, which owns a whole CU's LDS and holds maxefc rows of full length.
static bool rows_layout(Carver& cv, const UhcModelDesc& d, const KernelArgs& A, DevLds& F, TierCap& cp, int maxefc, int maxcon, int maxtwo, int budget_doubles, bool full_y) {
    const DevTopo& T = A.t;
    const int YS = T.maxdepth + 1;
    common_layout(cv, d, T, F, false);
    cp.maxefc = maxefc; cp.maxcon = maxcon; cp.ndense = T.ncpair > 0 ? maxtwo : 0;
    cp.ld_delta = (F.LD - A.lf.LD) * 8;
    F.con = cv.carve(std::max(maxcon * UHC_CON_STRIDE, cp.ndense * UHC_WAVE));
    F.dcol = F.con;  // (unused: see fast_layout)
    F.rowMisc = cv.carve(maxefc * 2);  // 4 ints per row; the collision pass keeps its candidate-pair list here (256 ints)
    F.ncon_nefc = cv.carve(2 + UHC_MAXTWO);  // ints: truncated flag, nefc, number of two-body rows, spare, their row ids, slot -> lane of the working set
    F.rowY = cv.carve(maxefc / 2 + 1);  // + the end of the last row
    F.rowR = cv.carve(maxefc); F.rowAref = cv.carve(maxefc); F.rowB = cv.carve(maxefc); F.rowF = cv.carve(maxefc); F.rowDa = cv.carve(maxefc); F.rowW = cv.carve(maxefc);
    // MPR walks hull vertices once per support call and lane: staged in LDS they cost an LDS read instead of an L2 round trip.  The
    // dense rows, their scalars and Yhat (contiguous) are not written before the collision pass is over: the vertices borrow them.
    F.dense = cv.carve(cp.ndense * A.nvp);
    F.dsc = cv.carve(cp.ndense * 4);  // (vel, jas, jaw, |Yhat|^2) of every dense row
    F.Y = cv.off;
    const int full = maxefc * YS + 8;
    int ycap = full_y ? full : std::min(budget_doubles - cv.off - (cv.guard_on ? 2 : 0), full);
    if (!full_y && ycap < 64 * 18) return false;  // too little left for rows: not worth a tier of its own
    if (ycap < cv.end1 - cv.off) ycap = cv.end1 - cv.off;     // (the region also holds the dynamics temporaries of phase 1)
    cp.ycap = ycap & ~1;
    cp.vstage = ((A.dbg & UHC_DEBUG_NO_VSTAGE) == 0 && T.ncpair > 0 && 3 * d.nmeshvert <= cp.ndense * A.nvp + cp.ndense * 4 + cp.ycap) ? F.dense : -1;
    cv.off += cp.ycap;
    cv.end_guard();
    F.total = cv.off;
    return cv.off <= budget_doubles;
}

// ---- tier 4 (huge): what the large tier cannot hold (more than 256 rows / 128 contacts / 32 body-body rows) or cannot finish (islands with
//      more force-carrying rows than a 64-row working set).  Persistent part + contacts + per-row scalars + the nv x nv Hessian of the
//      primal problem (packed lower triangle) in LDS; the Yhat rows themselves -- chain rows packed, body-body rows as dense nv-vectors --
//      in HBM (KernelArgs::gY / gD, one slice per env, L2-resident while the env's workgroup runs).  Rows: the largest multiple of 128 up
//      to UHC_HUGE_MAXEFC that the LDS holds (nv 75: 1024; nv 99, the humanoid among four boxes: 768).
static bool huge_layout(Carver& cv, const UhcModelDesc& d, const KernelArgs& A, DevLds& F, TierCap& cp, int maxefc, int maxcon) {
    const DevTopo& T = A.t;
    const int nv = d.nv, YS = T.maxdepth + 1;
    common_layout(cv, d, T, F, false);
    cp.maxefc = maxefc; cp.maxcon = maxcon; cp.ndense = T.ncpair > 0 ? UHC_HUGE_MAXTWO : 0;
    cp.ld_delta = (F.LD - A.lf.LD) * 8;
    // (after the rows are built the contacts' storage serves the Newton iteration: the dof-chain table, the run of chain rows the wave is adding
    //  to the Hessian, the dense group's D y, the pair table -- uhc_primal.h)
    const int scratch4 = primal_scratch(nv, YS).total;  // uhc_device.h: table | per-wave runs of rows | dense group | pair tables | run coefficients | mailbox
    F.con = cv.carve(std::max(cp.maxcon * UHC_CON_STRIDE, scratch4));
    F.dcol = F.con;
    F.rowMisc = cv.carve(std::max(maxefc * 2, 128));  // (the collision pass keeps its candidate-pair list here: 256 ints)
    F.ncon_nefc = cv.carve(2 + (cp.ndense + 1) / 2 + 1);  // ints: truncated flag, nefc, number of two-body rows, spare, their row ids
    F.rowY = cv.carve(maxefc / 2 + 1);
    F.rowR = cv.carve(maxefc); F.rowAref = cv.carve(maxefc); F.rowB = cv.carve(maxefc); F.rowF = cv.carve(maxefc); F.rowDa = cv.carve(maxefc); F.rowW = cv.carve(maxefc);
    F.dsc = cv.carve(std::max(cp.ndense * 4, 2));
    F.H = cv.carve((nv * (nv + 1)) / 2);
    F.Y = F.dense = F.H;  // (never addressed in this tier: the rows live in gY / gD)
    cp.ycap = maxefc * YS + 8;
    // MPR's hull vertices: staged where the Hessian will be (nothing of it exists during the collision pass) when they fit
    cp.vstage = ((A.dbg & UHC_DEBUG_NO_VSTAGE) == 0 && T.ncpair > 0 && 3 * d.nmeshvert <= (nv * (nv + 1)) / 2) ? F.H : -1;
    if (cv.off < cv.end1) cv.off = cv.end1;  // (the region also holds the dynamics temporaries of phase 1)
    cv.end_guard();
    F.total = cv.off;
    return cv.off <= 160 * 1024 / 8;
}

// the tiers behind the fast one: which exist (KernelArgs::last_tier) and their layouts; cv[1 .. 3] = general, large, tier 4
static int upper_tiers(Carver* cv, const UhcModelDesc& d, const BatchKnobs& knobs, BatchPlan& P, std::string* err) {
    KernelArgs& A = P.A;
    A.last_tier = knobs.tiers == 2 ? 2 : 3;
    if (A.last_tier == 3) {  // the large tier: as many rows (<= 256) as a CU's 160 KiB hold at full length
        bool ok = false;
        for (int me = UHC_BIG_MAXEFC; me > UHC_GEN_MAXEFC && !ok; me -= 32) {
            ok = rows_layout(cv[2], d, A, A.lh, A.ch, me, me / 2, UHC_BIG_MAXTWO, 160 * 1024 / 8, true);
        }
        if (ok) P.lds_bytes_big = (size_t)A.lh.total * sizeof(double);
        else A.last_tier = 2;
    }
    const int two_per_cu = 79 * 1024 / 8;
    bool ok = A.last_tier == 3 && rows_layout(cv[1], d, A, A.l, A.cg, UHC_GEN_MAXEFC, UHC_GEN_MAXCON, UHC_GEN_MAXTWO, two_per_cu, false);
    if (!ok) {  // the last tier must hold every row at full length: a whole CU's LDS if need be (32 dense slots as before)
        if (!rows_layout(cv[1], d, A, A.l, A.cg, UHC_GEN_MAXEFC, UHC_GEN_MAXCON, A.last_tier == 2 ? UHC_MAXTWO : UHC_GEN_MAXTWO, 160 * 1024 / 8, true))
            return refuse(err, "uhc_batch_create: model needs %zu B of LDS per env (> 160 KiB)", (size_t)A.l.total * 8);
    }
    P.lds_bytes = (size_t)A.l.total * sizeof(double);
    A.lx = A.lh; A.cx = A.ch; A.gY = A.gD = nullptr; A.gy_stride = A.gd_stride = 0;
    if (A.last_tier == 3 && knobs.tiers != 3) {  // (UHC_TIERS=3: the three-tier chain of rounds 3-4, windows and all)
        bool ok4 = false;
        // Rows and contacts share what the LDS has left beside the Hessian (128 rows = 8.7 KB = 45 contacts).  A contact brings at most four rows, a
        // body-body contact one; the extremes seen in 2.5 M env-steps of the ball-joint rollouts are 504 rows with 192+ contacts (2.6 rows per
        // contact) -- and 4 of those env-steps met a fixed 192-contact cap with 768 rows allotted.  So: for every row count that fits (multiples of
        // 128), the most contacts that fit beside it (>= UHC_HUGE_MAXCON, <= UHC_HUGE_MAXCON_MOST); the pair with the largest
        // min(rows / 2.75, contacts) wins (nv 99, the humanoid among four boxes: 640 rows / 237 contacts instead of 768 / 192).
        int best_me = 0, best_mc = 0;
        double best = -1.0;
        for (int me = UHC_HUGE_MAXEFC; me >= 384; me -= 128) {
            if (!huge_layout(cv[3], d, A, A.lx, A.cx, me, UHC_HUGE_MAXCON)) continue;
            int mc = UHC_HUGE_MAXCON_MOST;
            while (mc > UHC_HUGE_MAXCON && !huge_layout(cv[3], d, A, A.lx, A.cx, me, mc)) mc -= 8;
            const double score = std::min(me / 2.75, (double)mc);
            if (score > best) { best = score; best_me = me; best_mc = mc; }
        }
        ok4 = best_me > 0 && huge_layout(cv[3], d, A, A.lx, A.cx, best_me, best_mc);
        if (ok4 && (A.dbg & UHC_DEBUG_LOG)) fprintf(stderr, "uhc tier 4: %d rows / %d contacts / %d body-body rows, %d B of LDS\n", A.cx.maxefc, A.cx.maxcon, A.cx.ndense, A.lx.total * 8);
        if (ok4) {
            A.last_tier = 4;
            P.lds_bytes_big = std::max(P.lds_bytes_big, (size_t)A.lx.total * sizeof(double));
            A.gy_stride = A.cx.ycap;
            A.gd_stride = std::max(A.cx.ndense, 1) * A.nvp;
        } else { A.lx = A.lh; A.cx = A.ch; }
    }
    return 0;
}

// UHC_GUARD_LDS: per tier 64 ints -- [0] / [1] the number of guard words after the persistent / constraint-phase regions, [2 ..] / [32 ..] their offsets
static int guard_table(Carver* cv, const BatchKnobs& knobs, BatchPlan& P, std::string* err) {
    P.guard_tab.assign(4 * 64, 0);
    if (knobs.guard == 2) cv[0].persist.push_back(P.A.lf.qpos);
    for (int t = 0; t < 4; t++) {
        if (cv[t].persist.size() > 30 || cv[t].phase2.size() > 32) return refuse(err, "uhc_batch_create: UHC_GUARD_LDS: more guard words than the table holds");
        P.guard_tab[64 * t] = (int)cv[t].persist.size(); P.guard_tab[64 * t + 1] = (int)cv[t].phase2.size();
        for (size_t k = 0; k < cv[t].persist.size(); k++) P.guard_tab[64 * t + 2 + k] = cv[t].persist[k];
        for (size_t k = 0; k < cv[t].phase2.size(); k++) P.guard_tab[64 * t + 32 + k] = cv[t].phase2[k];
    }
    return 0;
}

// ------------------------------------------------------------------ schedules
// ---- static schedules for the factorisation and the triangular solves (see DevTopo).  Addresses are LDS byte
//      addresses of the FAST layout's LD buffer (the general kernel adds its own LD offset, KernelArgs::ld_delta).
static int schedules(const UhcModelDesc& d, BatchPlan& P, std::string* err) {
    KernelArgs& A = P.A;
    DevTopo& T = A.t;
    const int nv = d.nv, YS = T.maxdepth + 1;
    const std::vector<int>& dof_depth = P.dof_depth;
    // substitution tables: nv-1 steps, padded with no-op steps (zero-slot addresses) to a multiple of 8 plus one block of look-ahead
    const size_t sol_steps = (size_t)((std::max(nv - 1, 1) + 7) / 8 * 8 + 8);
    std::vector<unsigned int>& fac_prog = P.fac_prog;
    P.sol_back.assign(sol_steps * 64, 0); P.sol_fwd.assign(sol_steps * 64, 0);
    const unsigned ldb = (unsigned)A.lf.LD * 8u;
    auto adr = [&](int rel) { return ldb + 8u * (unsigned)rel; };
    const int ZERO = T.nM, DUMP = T.nM + 1;
    if (adr(DUMP) + 8 > 65536u || (unsigned)A.l.LD * 8u + 8u * (T.nM + 2) > 65536u) return refuse(err, "uhc_batch_create: LD buffer beyond the 16-bit schedule addresses");
    // factorisation program: a flat list of groups, one 24-byte record per lane and group (DevTopo::fac_prog).  A group holds three
    // 64-lane slots of updates of ONE elimination step k,  LD[row(anc_a) + t] -= (LD[kk + a] / D_k) * LD[kk + a + t],  the address of
    // D_k, and -- in the step's last group -- the lane's entry of row k to normalise (LD[kk + 1 + lane] /= D_k).  Steps need no
    // boundary handling in the kernel: the LDS queue of a wave is in order.
    int ngroups = 0;
    for (int k = nv - 1; k >= 1; k--) {
        const int dk = dof_depth[k], kk = d.dof_madr[k];
        if (!dk) continue;
        std::vector<unsigned> E;  // (af | ar << 16, ao) per entry
        int anc = k;
        for (int a = 1; a <= dk; a++) {
            anc = d.dof_parentid[anc];
            for (int t = 0; t <= dk - a; t++) { E.push_back(adr(kk + a) | (adr(kk + a + t) << 16)); E.push_back(adr(d.dof_madr[anc] + t)); }
        }
        constexpr int G = 3;  // update slots per group (uhc_physics.hip k_factor): 99 groups for the SMPL tree (129 with 2, 88 with 4 but 36 % more padded slots)
        while ((E.size() / 2) % (64 * G)) { E.push_back(adr(ZERO) | (adr(ZERO) << 16)); E.push_back(adr(DUMP)); }
        const int ng = (int)(E.size() / 2 / (64 * G));
        for (int gi = 0; gi < ng; gi++)
            for (int l = 0; l < 64; l++) {
                size_t e[G];
                for (int q = 0; q < G; q++) e[q] = ((size_t)gi * 64 * G + 64 * q + l) * 2;
                const unsigned nr = (gi == ng - 1 && l < dk) ? adr(kk + 1 + l) : adr(ZERO);
                for (int q = 0; q < G; q++) fac_prog.push_back(E[e[q]]);
                fac_prog.push_back(E[e[0] + 1] | (E[e[1] + 1] << 16));
                fac_prog.push_back(E[e[2] + 1] | (nr << 16));
                fac_prog.push_back(adr(kk));
            }
        ngroups += ng;
    }
    T.fac_nslot = ngroups;
    for (int q = 0; q < 2 * 64; q++) {  // two groups of look-ahead slack
        for (int w = 0; w < 3; w++) fac_prog.push_back(adr(ZERO) | (adr(ZERO) << 16));
        fac_prog.push_back(adr(DUMP) | (adr(DUMP) << 16)); fac_prog.push_back(adr(DUMP) | (adr(ZERO) << 16)); fac_prog.push_back(adr(ZERO));
    }
    auto entry = [&](int i, int j) -> unsigned {  // address of L[i][j] if j is a proper ancestor of i, else the zero slot
        if (i >= nv || j >= nv || j >= i || dof_depth[j] >= dof_depth[i]) return adr(ZERO);
        return P.dof_anc[(size_t)i * YS + dof_depth[j]] == j ? adr(d.dof_madr[i] + dof_depth[i] - dof_depth[j]) : adr(ZERO);
    };
    for (size_t q = 0; q < sol_steps * 64; q++) P.sol_back[q] = P.sol_fwd[q] = adr(ZERO) | (adr(ZERO) << 16);
    for (int s2 = 0; s2 < nv - 1; s2++)
        for (int l = 0; l < 64; l++) {
            const int i = nv - 1 - s2;
            P.sol_back[(size_t)s2 * 64 + l] = entry(i, l) | (entry(i, l + 64) << 16);
            P.sol_fwd[(size_t)s2 * 64 + l] = entry(l, s2) | (entry(l + 64, s2) << 16);
        }
    P.chain.assign((size_t)nv * 32, adr(0) << 16);
    for (int i = 0; i < nv; i++)
        for (int q = 0; q <= dof_depth[i]; q++) {
            const int a = P.dof_anc[(size_t)i * YS + q];
            P.chain[(size_t)i * 32 + q] = (unsigned)a | (adr(d.dof_madr[a]) << 16);
        }
    return 0;
}

// actuation is gathered per dof (lane = dof): up to UHC_DOF_MAXACT motors drive the joint of a dof (three on a ball joint, one per gear axis)
static int actuator_table(const UhcModelDesc& d, BatchPlan& P, std::string* err) {
    P.dof_act.assign((size_t)d.nv * UHC_DOF_MAXACT, -1);
    for (int a = 0; a < d.nu; a++) {
        const int j = d.dof_jntid[d.actuator_dofid[a]], nd = d.jnt_type[j] == UHC_JNT_BALL ? 3 : d.jnt_type[j] == UHC_JNT_FREE ? 6 : 1;
        if (nd == 6) return refuse(err, "uhc_batch_create: motors on free joints are not supported");
        for (int k = 0; k < nd; k++) {
            int q = 0;
            while (q < UHC_DOF_MAXACT && P.dof_act[(size_t)(d.jnt_dofadr[j] + k) * UHC_DOF_MAXACT + q] >= 0) q++;
            if (q == UHC_DOF_MAXACT) return refuse(err, "uhc_batch_create: more than %d motors on one joint", UHC_DOF_MAXACT);
            P.dof_act[(size_t)(d.jnt_dofadr[j] + k) * UHC_DOF_MAXACT + q] = a;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ the plan
#define PLAN_TRY(x) do { if (x) return 1; } while (0)
int plan_batch(const UhcModel* const* models, int n_models, const int32_t* env_model, int n_env, const UhcCtrlDesc* ctrl, const BatchKnobs& knobs,
               BatchPlan* out, std::string* err) {
    BatchPlan& P = *out;
    P = BatchPlan();
    if (knobs.fast_chunk_bad) return refuse(err, "uhc_batch_create: UHC_FAST_CHUNK must be a non-negative integer (substeps per chunk of the fast tier's control step)");
    PLAN_TRY(validate(models, n_models, env_model, n_env, ctrl, &P.n_trailing_free, err));
    const UhcModelDesc& d = models[0]->d;
    KernelArgs& A = P.A;
    memset(&A, 0, sizeof A);
    DevTopo& T = A.t;
    const int nv = d.nv;
    T.nq = d.nq; T.nv = nv; T.nu = d.nu; T.nbody = d.nbody; T.njnt = d.njnt; T.ngeom = d.ngeom; T.nmeshvert = d.nmeshvert;
    T.nM = d.dof_madr[nv];
    T.iterations = d.iterations; T.plane_mesh_maxcon = d.plane_mesh_maxcon; T.solver = d.solver;
    T.timestep = d.timestep; T.tolerance = d.tolerance;
    for (int k = 0; k < 3; k++) T.gravity[k] = d.gravity[k];
    T.has_damping = 0;
    for (int k = 0; k < n_models; k++)
        for (int i = 0; i < nv; i++) T.has_damping |= models[k]->d.dof_damping[i] > 0;
    for (int j = 0; j < d.njnt; j++) A.ball_limits |= d.jnt_type[j] == UHC_JNT_BALL && d.jnt_limited[j] != 0;
    A.n_env = n_env;
    tree_tables(d, P);
    PLAN_TRY(validate_trees(d, P, err));
    PLAN_TRY(collision_pairs(d, P, err));
    PLAN_TRY(model_blobs(models, n_models, P, err));
    PLAN_TRY(controller(d, ctrl, P, err));
    if (T.nM > 64 * 24) return refuse(err, "uhc_batch_create: nM %d > 1536 (the register tile that carries M between substeps)", T.nM);
    A.nvp = (nv + 1) & ~1;
    A.dbg = knobs.dbg;
    A.t4_rows = knobs.t4_rows;
    // sticky-tier marks: an env goes up a tier when it no longer fits (64 rows / 16 contacts / 12 body-body rows; the general tier's
    // capacities) and comes down again at 56 / 14 / 10 and at 7/8 of the general tier's.  Going up EARLIER (at 3/4 of a capacity, so
    // that no env finds out in mid-step) was measured on the self-colliding rollout: 51-55 k env-steps/s against 57 k -- the envs
    // parked a tier up cost more than the late hand-ons they avoid (profiles/r03_marks_sweep.txt)
    for (int k = 0; k < UHC_N_MARKS; k++) A.marks[k] = knobs.marks[k];  // (body-body rows, marks[UHC_MARK_UP2_TWO] < 0: set from the fast layout's dense slots unless UHC_TIER_MARKS names them)
    Carver cv[4];  // the layout being carved: 0 fast, 1 general, 2 large, 3 tier 4
    for (Carver& c : cv) c.guard_on = knobs.guard != 0;
    fast_layout(cv[0], d, n_env, knobs, P);
    PLAN_TRY(upper_tiers(cv, d, knobs, P, err));
    if (knobs.guard) PLAN_TRY(guard_table(cv, knobs, P, err));
    PLAN_TRY(schedules(d, P, err));
    PLAN_TRY(actuator_table(d, P, err));
    return 0;
}

// ------------------------------------------------------------------ the fast tier's launch in substep chunks
FastChunks plan_fast_chunks(int n_substeps, int chunk, int n_env) {
    FastChunks f;
    f.chunk = (chunk <= 0 || chunk >= n_substeps) ? 0 : chunk;
    f.n_chunks = f.chunk ? (n_substeps + f.chunk - 1) / f.chunk : 1;
    f.grid = f.n_chunks * n_env;
    f.prod_total = f.grid;
    return f;
}
void fast_chunk_range(const FastChunks& f, int n_substeps, int c, int* lo, int* hi) {
    *lo = f.chunk ? c * f.chunk : 0;
    *hi = f.chunk ? std::min(*lo + f.chunk, n_substeps) : n_substeps;
}
// UHC_FAST_CHUNK_DEFAULT substeps where the launch does not fit the chip at once: what does not fit starts when the first envs leave, a second round that
// leaves most places empty.  A batch that fits in one round gains nothing from chunks and pays their boundaries: the whole-step launch.
#define UHC_FAST_CHUNK_DEFAULT 5
int default_fast_chunk(int knob, int n_substeps, int n_env, int n_cu, size_t lds_bytes_fast) {
    if (knob > 0) return knob >= n_substeps ? 0 : knob;
    const int per_cu = std::max(1, std::min(4, (int)(160 * 1024 / std::max<size_t>(lds_bytes_fast, 1))));
    return (n_env > per_cu * n_cu && UHC_FAST_CHUNK_DEFAULT < n_substeps) ? UHC_FAST_CHUNK_DEFAULT : 0;
}

// ------------------------------------------------------------------ sticky tiers: one step's consumer launches
// tier 4's own consumers: when the newest counts seen say that envs went through tier 4 (est4: hand-ons of the large tier + envs that start there) while the
// general tier had a queue (est2_then: the consumers need the large tier's beside them, which run whenever the general tier's do), a few persistent workgroups
// wait on a queue of their own beside everything else, and the large tier's consumers append what they find too big instead of leaving it for the chained
// launch at the very end of the step -- where a 10 ms env-step of one env used to be added to every step in which any env needed tier 4 (configs[4]: 64 k ->
// 42 k env-steps/s when tier 4 came in).  Envs that START in tier 4 (UHC_DEBUG_EXP_STICKY_TIER4) are put at the head of that queue by the list kernel.
bool sticky_launch4(int last_tier, int est4, int est2_then, bool queues_off) { return last_tier == 4 && est4 > 0 && est2_then > 0 && !queues_off; }

StickySizes plan_sticky_step(const StickyInputs& in, bool launch4) {
    StickySizes s;
    s.fast = plan_fast_chunks(in.n_substeps, in.n_substeps > 0 ? default_fast_chunk(in.fast_chunk, in.n_substeps, in.n_env, in.n_cu, in.lds_bytes_fast) : 0, in.n_env);
    const int est2 = in.est2, est3 = in.est3, est4 = in.est4, n_env = in.n_env, n_cu = in.n_cu;
    const bool big = in.last_tier >= 3;  // (tier 4 has no chained launch of its own: the large tier's workgroups go on with it; under sticky tiers it has queue consumers)
    s.launch4 = launch4;  // (the list kernel's view; the consumers need the large tier's beside them: q4 below)
    // Three regimes.  No env in the general tier when last seen: no side launches, plain chain.  Up to three quarters of the batch
    // there: its launch is a CONSUMER that also waits for what the fast tier hands on while both run -- and is kept small enough that
    // the fast tier's workgroups always find LDS beside it (a consumer that holds all LDS while it waits for a launch that cannot
    // start would only end by its time-out).  The majority there: the fast tier is the side show; the general tier's launch takes
    // its list at full width and does not wait, what the fast tier hands on goes through the chained launch.
    s.queues = est2 > 0;
    s.waiting = s.queues && est2 <= (3 * n_env) / 4 && !in.queues_off;
    s.q3 = s.queues && big;  // (a large-tier consumer waits beside the general tier's launch whenever there is one: what that hands on is rare and slow)
    // (one waiting consumer per env expected in the queue: its own envs are done within one general-tier env-step and the consumers are
    //  free when the fast tier hands envs on.  Half as many -- more LDS for the fast tier, two envs in a row per consumer -- was
    //  measured on the self-colliding rollout: 59 k env-steps/s against 66 k)
    // The large tier's share of the chip: each of its workgroups holds a whole CU, two of the general tier's fit one.  With g3 CUs for
    // the large tier both queues take equally long when est3 / g3 = est2 / (2 (n_cu - g3)) (their env-steps last about as long); never
    // more consumers than envs expected, never fewer than 64 when there are that many envs.  (A fixed 64 was measured on the
    // ball_objects scene late in its cycle: 370 envs in the large tier's queue, six in a row per consumer, the step 61 ms of which the
    // general tier's launch took the first 20 -- tools/tier_trace.py --workload ball_objects.)
    const int share3 = est3 > 0 ? (int)((2ll * n_cu * est3) / std::max(1, est2 + 2 * est3)) : 0;
    // (beside a fast tier that still has most of the envs -- `waiting` -- the consumers are kept to a third of the chip: at most 32 CUs
    //  for the large tier, 256 workgroups of the general tier, 64 waiting spares.  Sized for their queues alone they left the fast tier 28
    //  CUs in the ball-joint rollout's first steps, and consumers that waited for it ran into their time-out.)
    s.grid3 = s.waiting ? std::min(est3 + est3 / 4 + 2, in.q3_max) : std::min(est3 + est3 / 4 + 2, std::max(64, std::min(share3, (3 * n_cu) / 4)));
    const int room2 = 2 * (n_cu - (in.large_first && s.q3 ? std::min(s.grid3, std::max(est3, 1)) : 0));  // general-tier workgroups beside the large tier's
    // (the cap grows with the general tier's share of the step's LDS-time: x consumers and s1 fast-tier workgroups on each of the
    //  remaining n_cu - x / 2 CUs take equally long when x = est2 s1 n_cu / (est1 + est2 s1 / 2) -- env-steps of the two tiers last
    //  about as long.  7/8 of that, never below UHC_Q2_MAX, never above 3/4 of the chip: 300 for configs[4] at 1024 envs, where 256 / 320 /
    //  384 consumers were measured at 65.5 / 66.5 k env-steps/s / worse.)
    const int s1 = std::max(1, std::min(4, (int)(160 * 1024 / std::max<size_t>(in.lds_bytes_fast, 1))));
    const int est1 = std::max(0, n_env - est2 - est3);
    const int bal = (int)(((long long)est2 * s1 * n_cu) / std::max(1, est1 + (est2 * s1) / 2));
    const int cap2 = in.fixed_cap2 ? in.q2_max : std::max(in.q2_max, std::min((7 * bal) / 8, (3 * n_cu) / 2));
    s.grid2 = s.waiting ? std::min(est2 / in.q2_div + 8, cap2) : std::min(est2 + est2 / 4 + 8, std::min(n_env, std::max(64, room2)));
    s.sticky_mask = (s.queues ? 4 : 0) | (s.q3 ? 8 : 0) | (s.launch4 ? 16 : 0);
    s.q4 = s.launch4 && s.q3;
    s.grid4 = std::min(in.q4_max, est4 + est4 / 2 + 2);
    // (seats for twice the hand-ons last seen: when the queue shrinks from step to step -- after a restart of many envs -- the launch
    //  is sized for a queue that is no longer there, and idle consumers that stay hold LDS the fast tier is waiting for: 150 of
    //  them made its last workgroups start 25 ms into the step on the ball-joint rollout's first steps)
    s.n_wait = std::min(64, std::max(in.q2_wait_min, 2 * in.handed2 + 8));
    return s;
}

// Who waits for whom: tier 4's consumers for the large tier's exits, the large tier's for the general tier's, the general tier's -- while the fast tier still
// has most of the envs (`waiting`) -- for the fast tier's; each tier hands on into the queue of the next one that has consumers this step.  A consumer of the
// large tier or tier 4 that finds its queue empty always waits (n_wait = grid, no seat counter); of the general tier's only n_wait do, counted in UHC_FIN_SPARES.
StepWiring sticky_wiring(const StickySizes& z, bool large_first) {
    StepWiring w{};
    auto add = [&](int tier, int stream, int grid) -> StepLaunch& {
        StepLaunch& l = w.launch[w.n++];
        l.tier = tier; l.stream = stream; l.grid = grid; l.prod_total = 0; l.n_wait = 0; l.gate_want = 0; l.tier_want = 0; l.chunk = 0; l.use_order = false;
        l.list = l.count = l.cursor = l.spares = l.started = l.prod_fin = l.fin = l.next_list = l.next_count = l.gate_started = l.gate_waited = UHC_NONE;
        return l;
    };
    if (z.q4) {  // (first of the side launches: a whole CU's LDS each, only to be had before the fast tier's launch has filled the chip)
        StepLaunch& l = add(4, STREAM_T4, z.grid4);
        l.list = UHC_LIST_T4; l.count = UHC_CNT_T4; l.cursor = UHC_CUR_T4; l.n_wait = z.grid4;
        l.prod_fin = UHC_FIN_BIG; l.prod_total = z.grid3;
    }
    auto large = [&]() {
        StepLaunch& l = add(3, STREAM_BIG, z.grid3);
        l.list = UHC_LIST_BIG; l.count = UHC_CNT_BIG; l.cursor = UHC_CUR_BIG; l.n_wait = z.grid3; l.started = UHC_FIN_BIG_IN;
        l.prod_fin = UHC_FIN_GEN; l.prod_total = z.grid2;  // the general tier's workgroups: they never wait for this launch
        if (z.q4) { l.fin = UHC_FIN_BIG; l.next_list = UHC_LIST_T4; l.next_count = UHC_CNT_T4; }
    };
    // (the large tier's consumers first where their stream has a queue pool of its own: whole CUs are only free while nothing else is resident, so the general
    //  tier's launch waits behind a gate until they have reported in)
    if (z.q3 && large_first) large();
    if (z.queues) {
        StepLaunch& l = add(2, STREAM_GEN, z.grid2);
        l.list = UHC_LIST_GEN; l.count = UHC_CNT_GEN; l.cursor = UHC_CUR_GEN; l.n_wait = z.n_wait; l.spares = UHC_FIN_SPARES; l.fin = UHC_FIN_GEN;
        if (z.waiting) { l.started = UHC_FIN_GEN_IN; l.prod_fin = UHC_FIN_FAST; l.prod_total = z.fast.prod_total; }  // every workgroup of the fast tier's launch
        if (z.q3) { l.next_list = UHC_LIST_BIG; l.next_count = UHC_CNT_BIG; }
        if (z.q3 && large_first) { l.gate_started = UHC_FIN_BIG_IN; l.gate_want = z.grid3; }
    }
    if (z.q3 && !large_first) large();
    // The fast tier's launch fills every CU's LDS the moment it starts; consumers that are not resident by then get theirs only when its first workgroups leave
    // (the tier trace showed them starting 3.7 ms into the step).  A one-thread gate on its stream holds the launch back until every consumer workgroup has
    // reported in (or 200 us have passed).
    StepLaunch& f = add(1, STREAM_MAIN, z.fast.grid);  // (in substep chunks: n_chunks x n_env workgroups, chunk-major by ticket)
    f.tier_want = 1; f.chunk = z.fast.chunk; f.use_order = true;  // (costliest envs first)
    if (z.waiting) {
        f.fin = UHC_FIN_FAST; f.next_list = UHC_LIST_GEN; f.next_count = UHC_CNT_GEN;
        f.gate_started = UHC_FIN_GEN_IN; f.gate_want = z.grid2; f.gate_waited = UHC_CNT_GATE_WAIT;
    }
    return w;
}
