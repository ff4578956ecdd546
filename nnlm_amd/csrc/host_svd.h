// host_svd.h -- host side of nnlm_svd / nnlm_get_svd / nnlm_set_factors_nndsvd(_batch): a part of nnlm_mi355x.hip, included there once,
// behind the launch helpers and the batch entries it builds on (it is not a header of its own: it uses that file's static functions).
// ---------------------------------------------------------------------------------------------
// Truncated SVD of the resident matrix and the NNDSVD start
// ---------------------------------------------------------------------------------------------
// Symmetric eigendecomposition of the l x l matrix a (row-major, destroyed): cyclic Jacobi in fp64, pairs (p, q) in row order, sweeps
// until the off-diagonal sum is exactly zero (Rutishauser's rules for a negligible entry).  lam descending, ties by index;
// E[r * l + i] = component r of eigenvector i.  A pure function of its input: no library, no threads.
static void jacobi_eigh(int l, std::vector<double> &a, std::vector<double> &lam, std::vector<double> &E)
{
    std::vector<double> v((size_t)l * l, 0.0);
    for (int i = 0; i < l; i++) v[(size_t)i * l + i] = 1.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0;
        for (int p = 0; p < l; p++)
            for (int q = p + 1; q < l; q++) off += fabs(a[(size_t)p * l + q]);
        if (off == 0.0) break;
        for (int p = 0; p < l; p++)
            for (int q = p + 1; q < l; q++) {
                const double apq = a[(size_t)p * l + q];
                if (apq == 0.0) continue;
                const double app = a[(size_t)p * l + p], aqq = a[(size_t)q * l + q], g = 100.0 * fabs(apq);
                if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    a[(size_t)p * l + q] = a[(size_t)q * l + p] = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < l; r++) { // columns p and q
                    const double rp = a[(size_t)r * l + p], rq = a[(size_t)r * l + q];
                    a[(size_t)r * l + p] = c * rp - s * rq;
                    a[(size_t)r * l + q] = s * rp + c * rq;
                }
                for (int r = 0; r < l; r++) { // rows p and q
                    const double pr = a[(size_t)p * l + r], qr = a[(size_t)q * l + r];
                    a[(size_t)p * l + r] = c * pr - s * qr;
                    a[(size_t)q * l + r] = s * pr + c * qr;
                }
                a[(size_t)p * l + q] = a[(size_t)q * l + p] = 0.0;
                for (int r = 0; r < l; r++) {
                    const double rp = v[(size_t)r * l + p], rq = v[(size_t)r * l + q];
                    v[(size_t)r * l + p] = c * rp - s * rq;
                    v[(size_t)r * l + q] = s * rp + c * rq;
                }
            }
    }
    std::vector<int> order(l);
    for (int i = 0; i < l; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * l + x] > a[(size_t)y * l + y]; });
    lam.resize(l);
    E.resize((size_t)l * l);
    for (int i = 0; i < l; i++) {
        lam[i] = a[(size_t)order[i] * l + order[i]];
        for (int r = 0; r < l; r++) E[(size_t)r * l + i] = v[(size_t)r * l + order[i]];
    }
}

// Test hook (nnlm_debug_set_svd_rotate): the form of the rotations of nnlm_svd, -1 = the width decides
static std::atomic<int> g_debug_svd_rotate{-1};

extern "C" int nnlm_debug_set_svd_rotate(int form)
{
    if (form != -1 && form != 0 && form != 8 && form != 16 && form != 32)
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_debug_set_svd_rotate: form must be -1 (the width decides), 32, 16, 8 or 0 (out of place), got %d", form);
    g_debug_svd_rotate = form;
    return NNLM_OK;
}

// Host time of one phase of nnlm_svd into h->svd_ms[slot]; with profiling on the phase's device work is waited for, so that the slot
// holds it (otherwise it is paid by the next wait)
struct SvdPhase {
    nnlm_handle *h;
    int slot;
    std::chrono::steady_clock::time_point t0;
    SvdPhase(nnlm_handle *h_, int slot_) : h(h_), slot(slot_), t0(std::chrono::steady_clock::now()) {}
    ~SvdPhase()
    {
        if (h->prof && slot < 3) hipStreamSynchronize(h->stream);
        h->svd_ms[slot] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

// The cross product of a half-step and nothing else: with the master of side `which`'s fixed factor Y (which = 1: W, 0: H) the other
// side's master becomes Y A (which = 1, [KP][mpad]) or Y A^T (which = 0, [KP][npad]).  The same launches as half_step's -- the split-fp16
// kernels in the fp32-operand mode, the strict ones otherwise, one launch per 64 rows beyond rank 64, the SpMM on a sparse handle --
// and the split-K slabs summed in slab order (slab_reduce_kernel) straight into the master.  No Gram, no sweep.
static int svd_cross(nnlm_handle *h, int which)
{
    SvdPhase ph(h, 0);
    const Side s = side_of(h, which);
    int S = 1;
    if (h->sparse) sp_cross(h, s);
    else {
        const HalfPlan p = plan_half(h, which, 0, 1, false);
        S = p.S;
        ProfScope ps(h, s.prof_xprod);
        if (h->x16) {
            prepare_factor16(h, s);
            h->fixed_maxw = h->maxbits;
            if (generic_rank(h)) {
                const int rc = launch_xprod_generic(h, s, p);
                if (rc != NNLM_OK) return rc;
            } else
                launch_xprod16(h, s, p);
        } else if (generic_rank(h)) {
            const int rc = launch_xprod_generic(h, s, p);
            if (rc != NNLM_OK) return rc;
        } else {
            if (which == 0) {
                const int rc = ensure_AT(h);
                if (rc != NNLM_OK) return rc;
            }
            launch_xprod_nkq(h, s, p);
        }
    }
    const size_t cnt = s.slab_stride;
    slab_reduce_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->Cx, S, cnt, which == 1 ? h->H64 : h->W64);
    LAUNCHCHK(h);
    return NNLM_OK;
}

// G = X X^T (l x l, fp64, row-major on the host) of the master of W (side = 0) or H (side = 1): gram_partial_kernel + fold
static int svd_gram(nnlm_handle *h, int side, int l, std::vector<double> &G)
{
    const int KP = h->KP;
    {
        SvdPhase ph(h, 1);
        ProfScope ps(h, P_GRAM);
        const Side s = side_of(h, side ^ 1); // (the view whose FIXED factor is that master)
        launch_gram(h, s, 0, s.p);
        LAUNCHCHK(h);
    }
    SvdPhase ph(h, 4);
    std::vector<double> buf((size_t)KP * KP);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(buf.data(), h->Graw, buf.size() * 8, hipMemcpyDeviceToHost));
    G.assign((size_t)l * l, 0.0);
    for (int i = 0; i < l; i++)
        for (int j = i; j < l; j++) G[(size_t)i * l + j] = G[(size_t)j * l + i] = buf[(size_t)i * KP + j]; // (the upper tiles are the computed ones)
    return NNLM_OK;
}

// master of W (side = 0) or H (side = 1) <- T X; T: l x l on the host, row-major
static int svd_rotate(nnlm_handle *h, int side, int l, const std::vector<double> &T, double *Tdev)
{
    const int KP = h->KP;
    std::vector<double> tp((size_t)KP * KP, 0.0);
    for (int i = 0; i < l; i++)
        for (int j = 0; j < l; j++) tp[(size_t)i * KP + j] = T[(size_t)i * l + j];
    {
        SvdPhase ph(h, 4);
        HIPCHK(h, hipStreamSynchronize(h->stream)); // (the previous rotation may still be reading Tdev: the last step rotates twice in a row)
        HIPCHK(h, hipMemcpy(Tdev, tp.data(), tp.size() * 8, hipMemcpyHostToDevice));
    }
    SvdPhase ph(h, 2);
    // the form the width asks for, or the test hook's (a tile that does not fit this width is not forced)
    int form = nnlm_svd_rotate_form(KP);
    const int forced = g_debug_svd_rotate.load(std::memory_order_relaxed);
    if (forced == 0 || (forced > 0 && nnlm_svd_rotate_rows(KP, forced) > 0)) form = forced;
    h->svd_form = form;
    double *X = side == 0 ? h->W64 : h->H64, *tmp = nullptr;
    const int ld = side == 0 ? h->npad : h->mpad;
    if (form == 0) HIPCHK(h, hipMalloc(&tmp, (size_t)KP * ld * 8)); // (out of place: widths beyond 1280, where a call is hours of host Jacobi anyway)
    hipError_t e = nnlm_tu_svd_rotate(X, ld, side == 0 ? h->n : h->m, KP, Tdev, form, tmp, h->stream);
    if (tmp) {
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        hipFree(tmp);
    }
    if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "nnlm_svd: the rotation at padded width %d (form %d): %s", KP, form, hipGetErrorString(e));
    LAUNCHCHK(h);
    return NNLM_OK;
}

// X <- orth(X), Gram-based, twice: G = X X^T = E L E^T, X <- diag(L_i^-1/2 where L_i > 1e-12 L_max, else 0) E^T X.  A direction that is
// dropped becomes a zero row.  Not Cholesky: X has rank below l whenever A has.
static int svd_orth(nnlm_handle *h, int side, int l, double *Tdev)
{
    std::vector<double> G, lam, E, T((size_t)l * l);
    for (int pass = 0; pass < 2; pass++) {
        int rc = svd_gram(h, side, l, G);
        if (rc != NNLM_OK) return rc;
        {
            SvdPhase ph(h, 3);
            jacobi_eigh(l, G, lam, E);
            const double lmax = lam[0];
            int kept = 0;
            for (int i = 0; i < l; i++) {
                const bool keep = lmax > 0.0 && lam[i] > 1e-12 * lmax;
                const double d = keep ? 1.0 / sqrt(lam[i]) : 0.0;
                kept += keep ? 1 : 0;
                for (int j = 0; j < l; j++) T[(size_t)i * l + j] = d * E[(size_t)j * l + i];
            }
            h->svd_kept = kept;
        }
        rc = svd_rotate(h, side, l, T, Tdev);
        if (rc != NNLM_OK) return rc;
    }
    return NNLM_OK;
}

static int svd_body(nnlm_handle *h, int l, unsigned power_iters, const double *omega, double **Tdev)
{
    int rc = NNLM_OK;
    {
        SvdPhase ph(h, 6);
        rc = set_factors_impl(h, l, nullptr, omega, nullptr, nullptr, 0); // H = Omega; W, Cx, red and the rest are the workspace
        if (rc != NNLM_OK) return rc;
        HIPCHK(h, hipMalloc(Tdev, (size_t)h->KP * h->KP * 8));
    }
    h->fuse_err = false;
    const int KP = h->KP;
    if ((rc = svd_cross(h, 0)) != NNLM_OK) return rc; // Y = Omega A^T
    if ((rc = svd_orth(h, 0, l, *Tdev)) != NNLM_OK) return rc;
    for (unsigned it = 0; it < power_iters; it++) {
        if ((rc = svd_cross(h, 1)) != NNLM_OK) return rc; // Z = Q A
        if ((rc = svd_orth(h, 1, l, *Tdev)) != NNLM_OK) return rc;
        if ((rc = svd_cross(h, 0)) != NNLM_OK) return rc; // Q = orth(Z A^T)
        if ((rc = svd_orth(h, 0, l, *Tdev)) != NNLM_OK) return rc;
    }
    if ((rc = svd_cross(h, 1)) != NNLM_OK) return rc; // B = Q A
    std::vector<double> G, lam, E, Tu((size_t)l * l), Tv((size_t)l * l);
    if ((rc = svd_gram(h, 1, l, G)) != NNLM_OK) return rc;
    {
        SvdPhase ph(h, 3);
        jacobi_eigh(l, G, lam, E);
        h->svd_sigma.assign(l, 0.0);
        const double lmax = lam[0];
        for (int i = 0; i < l; i++) {
            // (a direction the Gram cannot tell from rounding -- lambda at most 1e-12 lambda_max, the rule of orth -- has sigma = 0)
            const double sg = (lmax > 0.0 && lam[i] > 1e-12 * lmax) ? sqrt(lam[i]) : 0.0;
            h->svd_sigma[i] = sg;
            for (int j = 0; j < l; j++) {
                Tu[(size_t)i * l + j] = E[(size_t)j * l + i];
                Tv[(size_t)i * l + j] = sg > 0.0 ? E[(size_t)j * l + i] / sg : 0.0;
            }
        }
    }
    if ((rc = svd_rotate(h, 0, l, Tu, *Tdev)) != NNLM_OK) return rc; // U = V^T Q
    if ((rc = svd_rotate(h, 1, l, Tv, *Tdev)) != NNLM_OK) return rc; // Vt = Sigma^-1 V^T B
    SvdPhase ph(h, 4);
    HIPCHK(h, hipMalloc(&h->svdU, (size_t)KP * h->npad * 8));
    HIPCHK(h, hipMalloc(&h->svdVt, (size_t)KP * h->mpad * 8));
    HIPCHK(h, hipMemcpyAsync(h->svdU, h->W64, (size_t)KP * h->npad * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->svdVt, h->H64, (size_t)KP * h->mpad * 8, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->svd_l = l;
    h->svd_LP = KP;
    return NNLM_OK;
}

extern "C" int nnlm_svd(nnlm_handle *h, unsigned l_, unsigned power_iters, const double *omega)
{
    const char *who = "nnlm_svd";
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "%s: set the matrix first", who);
    if (h->sharded) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a handle with a communicator is not supported (the decomposition runs on one GPU)", who);
    if (h->sparse && h->sp_weighted) return weighted_refusal(h, who, "the truncated SVD (and the NNDSVD starts from it)");
    if (h->sparse && h->sp_missing)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a sparse matrix whose absent entries are missing has no SVD here (absent entries must be zeros)", who);
    if (h->holdout && h->ho_nnz > 0)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: the handle holds a hold-out set: its %lld held-out entries are missing entries", who, h->ho_nnz);
    if (h->any_missing) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: A has missing (NA, NaN or +-Inf) entries; the decomposition needs a finite A", who);
    const int lim = h->n < h->m ? h->n : h->m;
    if (l_ < 1 || l_ > (unsigned)lim) return fail(h, NNLM_ERR_ARG, "%s: sketch width l = %u outside 1 .. min(n, m) = %d", who, l_, lim);
    const int l = (int)l_;
    if (!omega) return fail(h, NNLM_ERR_ARG, "%s: omega is NULL (the caller supplies the l x m sketch matrix)", who);
    for (size_t e = 0; e < (size_t)l * h->m; e++)
        if (!std::isfinite(omega[e])) return fail(h, NNLM_ERR_ARG, "%s: omega[%zu] is not finite", who, e);
    HIPCHK(h, hipSetDevice(h->device));
    g_attr_err = hipSuccess;
    free_svd(h);
    for (double &t : h->svd_ms) t = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    double *Tdev = nullptr;
    const int rc = svd_body(h, l, power_iters, omega, &Tdev);
    sync_all(h);
    {
        SvdPhase ph(h, 6);
        hipFree(Tdev);
        free_factors(h); // the handle is left without factors, as after nnlm_set_matrix
    }
    if (rc != NNLM_OK) free_svd(h);
    h->svd_ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int nnlm_get_svd(nnlm_handle *h, unsigned k_, double *sigma, double *U, double *Vt)
{
    if (!h || h->svd_l < 1) return fail(h, NNLM_ERR_ARG, "nnlm_get_svd: no decomposition on the handle (call nnlm_svd first)");
    if (k_ < 1 || k_ > (unsigned)h->svd_l) return fail(h, NNLM_ERR_ARG, "nnlm_get_svd: k = %u outside 1 .. l = %d", k_, h->svd_l);
    HIPCHK(h, hipSetDevice(h->device));
    const int k = (int)k_, n = h->n, m = h->m, npad = h->npad, mpad = h->mpad;
    if (sigma) memcpy(sigma, h->svd_sigma.data(), (size_t)k * 8);
    if (U) { // n x k column-major: the rows of the resident copy
        std::vector<double> u((size_t)k * npad);
        HIPCHK(h, hipMemcpy(u.data(), h->svdU, u.size() * 8, hipMemcpyDeviceToHost));
        for (int q = 0; q < k; q++) memcpy(U + (size_t)q * n, &u[(size_t)q * npad], (size_t)n * 8);
    }
    if (Vt) { // k x m column-major
        std::vector<double> v((size_t)k * mpad);
        HIPCHK(h, hipMemcpy(v.data(), h->svdVt, v.size() * 8, hipMemcpyDeviceToHost));
        for (int j = 0; j < m; j++)
            for (int q = 0; q < k; q++) Vt[(size_t)j * k + q] = v[(size_t)q * mpad + j];
    }
    return NNLM_OK;
}

// NNDSVD (Boutsidis & Gallopoulos 2008) of the first kmax resident triplets: per component the side taken and the two scales
// (nndsvd_norms_kernel + the host's handful of square roots), and the fill of the variant (0: none, 1: mean(A))
static int nndsvd_components(nnlm_handle *h, const char *who, int kmax, int variant, std::vector<NndsvdRow> &comp, double *fill)
{
    HIPCHK(h, hipSetDevice(h->device));
    const int n = h->n, m = h->m;
    const int nb = nnlm_nndsvd_norm_blocks(n, m);
    const bool need_mean = variant == 1 && !h->svd_mean_known;
    const size_t cnt = h->sparse ? (size_t)h->nnz : (size_t)h->npad * h->mpad; // (the padding of the dense layout is zeros)
    const size_t sb = need_mean ? nnlm_svd_sum_scratch(cnt) : 0;
    double *dev = nullptr;
    const size_t part = (size_t)kmax * nb * 4, elems = part + 4 * (size_t)kmax + sb + 1;
    HIPCHK(h, hipMalloc(&dev, elems * 8));
    nnlm_tu_nndsvd_norms(h->svdU, h->npad, n, h->svdVt, h->mpad, m, kmax, dev, dev + part, h->stream);
    if (need_mean) nnlm_tu_svd_sum(h->sparse ? h->sp_cval : h->A, h->prec == NNLM_PREC_F64, cnt, dev + part + 4 * kmax + 1, dev + part + 4 * kmax, h->stream);
    std::vector<double> out(4 * (size_t)kmax + 1, 0.0);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(out.data(), dev + part, (4 * (size_t)kmax + (need_mean ? 1 : 0)) * 8, hipMemcpyDeviceToHost);
    hipFree(dev);
    if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "%s: the NNDSVD norms failed: %s", who, hipGetErrorString(e));
    if (need_mean) {
        h->svd_mean = out[4 * (size_t)kmax] / ((double)n * (double)m);
        h->svd_mean_known = true;
    }
    *fill = variant == 1 ? h->svd_mean : 0.0;
    comp.resize(kmax);
    for (int j = 0; j < kmax; j++) {
        const double sg = h->svd_sigma[j];
        NndsvdRow &c = comp[j];
        c.src = j;
        if (j == 0) {
            c.side = 0;
            c.su = c.sv = sqrt(sg);
            continue;
        }
        const double up = sqrt(out[4 * j]), un = sqrt(out[4 * j + 1]), vp = sqrt(out[4 * j + 2]), vn = sqrt(out[4 * j + 3]);
        const double pp = up * vp, gg = un * vn;
        const bool pos = pp >= gg;
        const double t = pos ? pp : gg, nu = pos ? up : un, nv = pos ? vp : vn;
        c.side = pos ? 1 : -1;
        const double st = sg * t;
        if (st > 0.0) c.su = sqrt(st) / nu, c.sv = sqrt(st) / nv;
        else c.su = c.sv = 0.0; // (a zero column and row, never 0 / 0)
    }
    return NNLM_OK;
}

// The start into the masters (and the fp32 copy of W) of the factors just allocated at rank h->k: row r from component src[r] (-1: zeros)
static int nndsvd_build(nnlm_handle *h, const char *who, const std::vector<NndsvdRow> &comp, const std::vector<int> &src, double fill)
{
    const int KP = h->KP;
    std::vector<NndsvdRow> rows(KP);
    for (int r = 0; r < KP; r++) {
        if (r < (int)src.size() && src[r] >= 0) rows[r] = comp[src[r]];
        else rows[r] = NndsvdRow{-1, 0, 0.0, 0.0};
    }
    NndsvdRow *dev = nullptr;
    HIPCHK(h, hipMalloc(&dev, rows.size() * sizeof(NndsvdRow)));
    hipError_t e = hipMemcpy(dev, rows.data(), rows.size() * sizeof(NndsvdRow), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        nnlm_tu_nndsvd_build(h->svdU, h->npad, h->svdVt, h->mpad, dev, KP, fill, h->W64, h->prec == NNLM_PREC_F64 ? nullptr : (float *)h->Wop, h->npad,
                             h->n, h->H64, h->mpad, h->m, h->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(dev);
    if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "%s: nndsvd_build_kernel failed: %s", who, hipGetErrorString(e));
    return NNLM_OK;
}

static int nndsvd_refusal(nnlm_handle *h, const char *who, unsigned kmax, int variant)
{
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "%s: set the matrix first", who);
    if (h->sparse && h->sp_weighted) return weighted_refusal(h, who, "an NNDSVD start");
    if (h->svd_l < 1) return fail(h, NNLM_ERR_ARG, "%s: no decomposition on the handle (call nnlm_svd first)", who);
    if (variant != 0 && variant != 1) return fail(h, NNLM_ERR_ARG, "%s: variant must be 0 (nndsvd) or 1 (nndsvda), got %d", who, variant);
    if (kmax > (unsigned)h->svd_l) return fail(h, NNLM_ERR_ARG, "%s: rank %u exceeds the sketch width l = %d of the decomposition", who, kmax, h->svd_l);
    return NNLM_OK;
}

extern "C" int nnlm_set_factors_nndsvd(nnlm_handle *h, unsigned k_, int variant)
{
    const char *who = "nnlm_set_factors_nndsvd";
    int rc = nndsvd_refusal(h, who, k_, variant);
    if (rc != NNLM_OK) return rc;
    if (k_ < 1) return fail(h, NNLM_ERR_ARG, "%s: rank k must be >= 1", who);
    const int k = (int)k_;
    std::vector<NndsvdRow> comp;
    double fill = 0.0;
    if ((rc = nndsvd_components(h, who, k, variant, comp, &fill)) != NNLM_OK) return rc;
    if ((rc = factors_alloc(h, k, 0)) != NNLM_OK) return rc;
    std::vector<int> src(k);
    for (int q = 0; q < k; q++) src[q] = q;
    if ((rc = nndsvd_build(h, who, comp, src, fill)) != NNLM_OK) return rc;
    return factors_masks(h, k, nullptr, nullptr);
}

extern "C" int nnlm_set_factors_nndsvd_batch(nnlm_handle *h, unsigned B, const unsigned *k, int variant)
{
    const char *who = "nnlm_set_factors_nndsvd_batch";
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "%s: set the matrix first", who);
    int rc = batch_ranks(h, who, "members and their ranks", B, k, [&] { return batch_refusal(h, who); });
    if (rc != NNLM_OK) return rc;
    unsigned kmax = 0;
    for (unsigned b = 0; b < B; b++) kmax = k[b] > kmax ? k[b] : kmax;
    if ((rc = nndsvd_refusal(h, who, kmax, variant)) != NNLM_OK) return rc;
    std::vector<int> off(B + 1, 0);
    for (unsigned b = 0; b < B; b++) off[b + 1] = off[b] + (int)k[b];
    const int K = off[B];
    std::vector<NndsvdRow> comp;
    double fill = 0.0;
    if ((rc = nndsvd_components(h, who, (int)kmax, variant, comp, &fill)) != NNLM_OK) return rc;
    if ((rc = factors_alloc(h, K, 64)) != NNLM_OK) return rc;
    std::vector<int> src(K);
    for (unsigned b = 0; b < B; b++)
        for (unsigned q = 0; q < k[b]; q++) src[off[b] + q] = (int)q; // member b: the first k_b triplets, at its rows off_b ..
    if ((rc = nndsvd_build(h, who, comp, src, fill)) != NNLM_OK) return rc;
    if ((rc = factors_masks(h, K, nullptr, nullptr)) != NNLM_OK) return rc;
    return batch_setup(h, B, k, off);
}

