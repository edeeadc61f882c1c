/*
 * pbd_oracle_impl.inc -- type-generic body of the CPU oracle.  Included twice by pbd_oracle.c with
 *   REAL = float  / FN(x) = x##_f32   (reference T=float)
 *   REAL = double / FN(x) = x##_f64   (reference T=double)
 * TEST INFRASTRUCTURE ONLY (see pbd_oracle.h).  PARITY UNPINNED (see pbd_oracle.h).
 *
 * Every mixed float/double expression is written with explicit casts so that it evaluates exactly
 * as the reference's C++ does for that T; the file is compiled with -ffp-contract=off.
 */

#ifndef REAL
#error "include from pbd_oracle.c"
#endif

/* ------------------------------------------------------------------------------------------
 * HOG features of one image.  Follows src/HOGFeatures.cpp:168-341 (features<uint8_t>).
 * feat: out_rows x (out_cols*flen), channel fastest, zero-initialised here.
 * ---------------------------------------------------------------------------------------- */
/* IT-typed difference of two pixels, converted to T: `*(s+a) - *(s-b)` of features<IT> (:209-233): integer pixels
 * are promoted to int, float / double pixels subtract in their own type */
static inline REAL FN(pix_diff)(const void *im, int depth, size_t ia, size_t ib)
{
    switch (depth) {
    case PBDO_16U: return (REAL)((int)((const uint16_t *)im)[ia] - (int)((const uint16_t *)im)[ib]);
    case PBDO_32F: return (REAL)(((const float *)im)[ia] - ((const float *)im)[ib]);
    case PBDO_64F: return (REAL)(((const double *)im)[ia] - ((const double *)im)[ib]);
    default: return (REAL)((int)((const uint8_t *)im)[ia] - (int)((const uint8_t *)im)[ib]);
    }
}

void FN(pbdo_hog_features_d)(const void *im, int depth, int rows, int cols, int cn, size_t stride,
                             int sbin, int norient, int flen, REAL *feat);
void FN(pbdo_hog_features)(const uint8_t *im, int rows, int cols, int cn, size_t stride,
                           int sbin, int norient, int flen, REAL *feat)
{
    FN(pbdo_hog_features_d)(im, PBDO_8U, rows, cols, cn, stride, sbin, norient, flen, feat);
}

/* stride in elements of the image depth */
void FN(pbdo_hog_features_d)(const void *im, int depth, int rows, int cols, int cn, size_t stride,
                             int sbin, int norient, int flen, REAL *feat)
{
    /* :174-176 */
    const int bw = (int)roundf((float)cols / (float)sbin);
    const int bh = (int)roundf((float)rows / (float)sbin);
    const int ow = bw - 2 > 0 ? bw - 2 : 0;
    const int oh = bh - 2 > 0 ? bh - 2 : 0;
    const int visw = bw * sbin, vish = bh * sbin;
    const int half = norient / 2;

    REAL *hist = (REAL *)calloc((size_t)(bh > 0 ? bh : 1) * (size_t)(bw > 0 ? bw : 1) * norient, sizeof(REAL));
    REAL *norm = (REAL *)calloc((size_t)(bh > 0 ? bh : 1) * (size_t)(bw > 0 ? bw : 1), sizeof(REAL));
    memset(feat, 0, (size_t)oh * ow * flen * sizeof(REAL));
    const size_t histstride = (size_t)bw * norient;
    const size_t normstride = (size_t)bw;
    const size_t featstride = (size_t)ow * flen;

    const double eps = 0.0001; /* :189 */
    /* :192-193 (double literals converted to T) */
    const REAL uu[9] = {(REAL)1.000, (REAL)0.9397, (REAL)0.7660, (REAL)0.5000, (REAL)0.1736,
                        (REAL)-0.1736, (REAL)-0.5000, (REAL)-0.7660, (REAL)-0.9397};
    const REAL vv[9] = {(REAL)0.000, (REAL)0.3420, (REAL)0.6428, (REAL)0.8660, (REAL)0.9848,
                        (REAL)0.9848, (REAL)0.8660, (REAL)0.6428, (REAL)0.3420};

    /* :202-267 */
    for (int y = 1; y < vish - 1; ++y) {
        for (int x = 1; x < visw - 1; ++x) {
            REAL dx, dy, v;
            const int xs = x < cols - 2 ? x : cols - 2;
            const int ys = y < rows - 2 ? y : rows - 2;
            if (cn == 1) { /* :207-212 */
                const size_t s = (size_t)xs + (size_t)ys * stride;
                dy = FN(pix_diff)(im, depth, s + stride, s - stride);
                dx = FN(pix_diff)(im, depth, s + 1, s - 1);
                v = dx * dx + dy * dy;
            } else { /* :217-240 */
                size_t s = 3 * (size_t)xs + (size_t)ys * stride;
                REAL dyb = FN(pix_diff)(im, depth, s + stride, s - stride);
                REAL dxb = FN(pix_diff)(im, depth, s + 3, s - 3);
                REAL vb = dxb * dxb + dyb * dyb;
                s += 1;
                REAL dyg = FN(pix_diff)(im, depth, s + stride, s - stride);
                REAL dxg = FN(pix_diff)(im, depth, s + 3, s - 3);
                REAL vg = dxg * dxg + dyg * dyg;
                s += 1;
                dy = FN(pix_diff)(im, depth, s + stride, s - stride);
                dx = FN(pix_diff)(im, depth, s + 3, s - 3);
                v = dx * dx + dy * dy;
                if (vg > v) { v = vg; dx = dxg; dy = dyg; }
                if (vb > v) { v = vb; dx = dxb; dy = dyb; }
            }
            /* :243-249 */
            REAL best_dot = 0;
            int best_o = 0;
            for (int o = 0; o < half; ++o) {
                REAL dot = uu[o] * dx + vv[o] * dy;
                if (dot > best_dot) { best_dot = dot; best_o = o; }
                else if (-dot > best_dot) { best_dot = -dot; best_o = o + half; }
            }
            /* :252-260  (T)y+0.5 etc. are evaluated in double and rounded once to T */
            REAL yp = (REAL)(((double)(REAL)y + 0.5) / (double)(REAL)sbin - 0.5);
            REAL xp = (REAL)(((double)(REAL)x + 0.5) / (double)(REAL)sbin - 0.5);
            int iyp = (int)floor((double)yp);
            int ixp = (int)floor((double)xp);
            REAL vy0 = yp - (REAL)iyp;
            REAL vx0 = xp - (REAL)ixp;
            REAL vy1 = (REAL)(1.0 - (double)vy0);
            REAL vx1 = (REAL)(1.0 - (double)vx0);
            v = (REAL)SQRT_REAL(v);
            /* :262-265 */
            if (iyp >= 0 && ixp >= 0)
                hist[iyp * histstride + (size_t)ixp * norient + best_o] += vy1 * vx1 * v;
            if (iyp >= 0 && ixp + 1 < bw)
                hist[iyp * histstride + (size_t)(ixp + 1) * norient + best_o] += vx0 * vy1 * v;
            if (iyp + 1 < bh && ixp >= 0)
                hist[(size_t)(iyp + 1) * histstride + (size_t)ixp * norient + best_o] += vy0 * vx1 * v;
            if (iyp + 1 < bh && ixp + 1 < bw)
                hist[(size_t)(iyp + 1) * histstride + (size_t)(ixp + 1) * norient + best_o] += vy0 * vx0 * v;
        }
    }

    /* :270-283 */
    for (int y = 0; y < bh; ++y) {
        const REAL *src = hist + y * histstride;
        REAL *dst = norm + y * normstride;
        for (int x = 0; x < bw; ++x) {
            REAL acc = 0;
            for (int o = 0; o < half; ++o) {
                REAL t = src[o] + src[o + half];
                acc += t * t;
            }
            dst[x] = acc;
            src += norient;
        }
    }

    /* :286-340 */
    for (int y = 0; y < oh; ++y) {
        for (int x = 0; x < ow; ++x) {
            REAL *dst = feat + y * featstride + (size_t)x * flen;
            const REAL *p;
            REAL n1, n2, n3, n4;
            p = norm + (size_t)(y + 1) * normstride + (x + 1);
            n1 = (REAL)((double)1.0f / sqrt((double)(((p[0] + p[1]) + p[normstride]) + p[normstride + 1]) + eps));
            p = norm + (size_t)y * normstride + (x + 1);
            n2 = (REAL)((double)1.0f / sqrt((double)(((p[0] + p[1]) + p[normstride]) + p[normstride + 1]) + eps));
            p = norm + (size_t)(y + 1) * normstride + x;
            n3 = (REAL)((double)1.0f / sqrt((double)(((p[0] + p[1]) + p[normstride]) + p[normstride + 1]) + eps));
            p = norm + (size_t)y * normstride + x;
            n4 = (REAL)((double)1.0f / sqrt((double)(((p[0] + p[1]) + p[normstride]) + p[normstride + 1]) + eps));

            REAL t1 = 0, t2 = 0, t3 = 0, t4 = 0;
            const REAL lim = (REAL)0.2;
            const REAL *src = hist + (size_t)(y + 1) * histstride + (size_t)(x + 1) * norient;
            for (int o = 0; o < norient; ++o) { /* :304-317 */
                REAL val = src[o];
                REAL h1 = val * n1; if (lim < h1) h1 = lim;
                REAL h2 = val * n2; if (lim < h2) h2 = lim;
                REAL h3 = val * n3; if (lim < h3) h3 = lim;
                REAL h4 = val * n4; if (lim < h4) h4 = lim;
                *(dst++) = (REAL)(0.5 * (double)(((h1 + h2) + h3) + h4));
                t1 += h1; t2 += h2; t3 += h3; t4 += h4;
            }
            for (int o = 0; o < half; ++o) { /* :320-329 */
                REAL sum = src[o] + src[o + half];
                REAL h1 = sum * n1; if (lim < h1) h1 = lim;
                REAL h2 = sum * n2; if (lim < h2) h2 = lim;
                REAL h3 = sum * n3; if (lim < h3) h3 = lim;
                REAL h4 = sum * n4; if (lim < h4) h4 = lim;
                *(dst++) = (REAL)(0.5 * (double)(((h1 + h2) + h3) + h4));
            }
            /* :332-338 */
            *(dst++) = (REAL)(0.2357 * (double)t1);
            *(dst++) = (REAL)(0.2357 * (double)t2);
            *(dst++) = (REAL)(0.2357 * (double)t3);
            *(dst++) = (REAL)(0.2357 * (double)t4);
            *dst = 0;
        }
    }
    free(hist);
    free(norm);
}

/* ------------------------------------------------------------------------------------------
 * "Same"-size correlation of one feature level with one filter.
 * Follows src/SpatialConvolutionEngine.cpp:70-94 (split into planes, per-plane FilterEngine::apply,
 * pdf += pdfc for c = 0..flen-1), :141-158 (constant border 0, but 1 for the last channel, anchor
 * at the kernel centre) and src/filter.cpp:3808-3857 (tap list = non-zero coefficients in raster
 * order), :3916-3922 / :2186-2227 (s = delta(0); s += kf[k]*src_k, separate multiply and add).
 * The planes are materialised with their constant border, as FilterEngine does, and every tap is
 * applied to a whole output row at a time (the SSE loop order); per output element the sequence of
 * operations is exactly s = ((0 + w0*v0) + w1*v1) + ..., then resp = ((0 + s_0) + s_1) + ...
 * ---------------------------------------------------------------------------------------- */
void FN(pbdo_conv)(const REAL *feat, int H, int W, int flen, const REAL *filt, int k, REAL *resp)
{
    const int a = k / 2; /* normalizeAnchor(Point(-1,-1)) -> ksize/2 */
    const int PH = H + k - 1, PW = W + k - 1;
    REAL *plane = (REAL *)malloc((size_t)PH * PW * sizeof(REAL));
    REAL *acc = (REAL *)malloc((size_t)W * sizeof(REAL));
    for (size_t i = 0; i < (size_t)H * W; ++i) resp[i] = 0; /* pdf = Mat::zeros */
    for (int c = 0; c < flen; ++c) {
        const REAL border = (c == flen - 1) ? (REAL)1 : (REAL)0;
        /* split(): channel c as a bordered plane */
        for (int y = 0; y < PH; ++y) {
            REAL *prow = plane + (size_t)y * PW;
            const int yy = y - a;
            if (yy < 0 || yy >= H) {
                for (int x = 0; x < PW; ++x) prow[x] = border;
            } else {
                for (int x = 0; x < a; ++x) prow[x] = border;
                const REAL *frow = feat + ((size_t)yy * W) * flen + c;
                for (int x = 0; x < W; ++x) prow[a + x] = frow[(size_t)x * flen];
                for (int x = a + W; x < PW; ++x) prow[x] = border;
            }
        }
        int nz = 0;
        for (int i = 0; i < k * k; ++i) nz += (filt[(size_t)i * flen + c] != 0);
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x) acc[x] = 0; /* s = delta */
            if (nz == 0) {
                /* preprocess2DKernel keeps one zero tap at (0,0): s += 0*src */
                const REAL *srow = plane + (size_t)y * PW;
                for (int x = 0; x < W; ++x) acc[x] += (REAL)0 * srow[x];
            } else {
                for (int i = 0; i < k; ++i) {
                    for (int j = 0; j < k; ++j) {
                        const REAL w = filt[((size_t)i * k + j) * flen + c];
                        if (w == 0) continue;
                        const REAL *srow = plane + (size_t)(y + i) * PW + j;
                        for (int x = 0; x < W; ++x) acc[x] += w * srow[x];
                    }
                }
            }
            REAL *rrow = resp + (size_t)y * W;
            for (int x = 0; x < W; ++x) rrow[x] += acc[x]; /* pdf += pdfc */
        }
    }
    free(plane);
    free(acc);
}

/* ------------------------------------------------------------------------------------------
 * Generalised distance transform.  include/DistanceTransform.hpp:89-105 (Quadratic),
 * :152-182 (computeRow), :203-245 (compute incl. the Iy composition at :233-244).
 * ---------------------------------------------------------------------------------------- */
static inline double FN(quad_isect)(double a, double b, int x0, int x1, double y0, double y1)
{ /* :98-100 */
    return ((y1 - y0) - b * (double)(x1 - x0) + a * (double)(x1 * x1 - x0 * x0)) / (2 * a * (double)(x1 - x0));
}
static inline double FN(quad_val)(double a, double b, int x, double y)
{ /* :103-105 */
    return a * (double)(x * x) + b * (double)x + y;
}

static void FN(dt_row)(const REAL *src, REAL *dst, int *ptr, int N, double a, double b, int os,
                       int *v, REAL *z)
{ /* :152-182 */
    int k = 0;
    long long nan_pushed = 0; /* intersections pushed as NaN: a later s <= z[k] is false, so such an entry is never popped */
    v[0] = 0;
    z[0] = -(REAL)INFINITY;
    z[1] = (REAL)INFINITY;
    for (int q = 1; q < N; ++q) {
        REAL s = (REAL)FN(quad_isect)(a, b, v[k], q, (double)src[v[k]], (double)src[q]);
        while (s <= z[k] && k > 0) {
            k--;
            s = (REAL)FN(quad_isect)(a, b, v[k], q, (double)src[v[k]], (double)src[q]);
        }
        k++;
        v[k] = q;
        z[k] = s;
        z[k + 1] = (REAL)INFINITY;
        nan_pushed += (s != s);
    }
    if (nan_pushed) {
#pragma omp atomic
        pbdo_nan_isect_count += nan_pushed;
    }
    if (pbdo_dt_readout == PBDO_READOUT_MAX) {
        /* the project's rule for envelopes that hold a NaN intersection (include/pbd.h, pbd_dp_min): position q takes entry
         * max{k : z[k] < os + q}, a comparison with NaN being false.  That set shrinks as q falls, so one walk down from the
         * top serves every q; z[0] = -inf ends it.  Where z[1..top] is non-decreasing and NaN-free this is the loop below. */
        for (int q = N - 1; q >= 0; --q) {
            while (!(z[k] < (REAL)(os + q))) k--;
            dst[q] = (REAL)FN(quad_val)(a, b, os + q - v[k], (double)src[v[k]]);
            ptr[q] = v[k];
        }
        return;
    }
    k = 0;
    for (int q = 0; q < N; ++q) {
        while (z[k + 1] < (REAL)os) k++;
        dst[q] = (REAL)FN(quad_val)(a, b, os - v[k], (double)src[v[k]]);
        ptr[q] = v[k];
        os++;
    }
}

void FN(pbdo_dt)(const REAL *in, int M, int N, double ax, double bx, double ay, double by,
                 int osx, int osy, REAL *out, int *Ix, int *Iy)
{
    const int L = (M > N ? M : N);
    int *v = (int *)malloc((size_t)L * sizeof(int));
    REAL *z = (REAL *)malloc((size_t)(L + 1) * sizeof(REAL));
    REAL *tmp = (REAL *)malloc((size_t)M * N * sizeof(REAL));
    REAL *col_in = (REAL *)malloc((size_t)M * sizeof(REAL));
    REAL *col_out = (REAL *)malloc((size_t)M * sizeof(REAL));
    int *col_ptr = (int *)malloc((size_t)M * sizeof(int));
    int *row = (int *)malloc((size_t)N * sizeof(int));

    for (int m = 0; m < M; ++m) /* :216-218 */
        FN(dt_row)(in + (size_t)m * N, tmp + (size_t)m * N, Ix + (size_t)m * N, N, ax, bx, osx, v, z);
    for (int n = 0; n < N; ++n) { /* :221-231: transpose, column pass, transpose back */
        for (int m = 0; m < M; ++m) col_in[m] = tmp[(size_t)m * N + n];
        FN(dt_row)(col_in, col_out, col_ptr, M, ay, by, osy, v, z);
        for (int m = 0; m < M; ++m) {
            out[(size_t)m * N + n] = col_out[m];
            Iy[(size_t)m * N + n] = col_ptr[m];
        }
    }
    for (int m = 0; m < M; ++m) { /* :233-244 */
        int *Iy_ptr = Iy + (size_t)m * N;
        const int *Ix_ptr = Ix + (size_t)m * N;
        for (int n = 0; n < N; ++n) row[n] = Iy_ptr[Ix_ptr[n]];
        for (int n = 0; n < N; ++n) Iy_ptr[n] = row[n];
    }
    free(v); free(z); free(tmp); free(col_in); free(col_out); free(col_ptr); free(row);
}

/* ------------------------------------------------------------------------------------------
 * DynamicProgram<T>::min for one (level, component).  src/DynamicProgram.cpp:83-171,
 * include/Math.hpp:149-185 (reduceMax), :109-135 (reducePickIndex), include/Parts.hpp:172-187.
 * ---------------------------------------------------------------------------------------- */
void FN(pbdo_dp_min)(const pbdo_model *m, int c, const REAL *responses, int H, int W,
                     int *Ix, int *Iy, int *Ik, REAL *rootv, int *rooti)
{
    const size_t HW = (size_t)H * W;
    const int p0 = m->part_offset[c];
    const int nparts = m->part_offset[c + 1] - p0;
    int *slots = (int *)malloc(sizeof(int) * (size_t)m->part_offset[m->ncomponents]);
    pbdo_ptr_slots(m, slots);

    /* ncscores: lazily materialised copies keyed by filter id (:93, :154-155) */
    REAL **nc = (REAL **)calloc((size_t)m->nfilters, sizeof(REAL *));

    for (int p = nparts - 1; p > 0; --p) { /* :95 */
        const int gp = p0 + p;
        const int K = m->mix_offset[gp + 1] - m->mix_offset[gp];
        const int gpar = p0 + m->parentid[gp];
        const int L = m->mix_offset[gpar + 1] - m->mix_offset[gpar];
        REAL *scoresp = (REAL *)malloc(sizeof(REAL) * HW * K);
        int *Ixp = (int *)malloc(sizeof(int) * HW * K);
        int *Iyp = (int *)malloc(sizeof(int) * HW * K);
        for (int mm = 0; mm < K; ++mm) { /* :110-132 */
            const int gm = m->mix_offset[gp] + mm;
            const int f = m->filterid[gm];
            const REAL *score_in = nc[f] ? nc[f] : responses + (size_t)f * HW;
            const int d = m->defid[gm];
            const float *w = m->defw + (size_t)d * 4;
            FN(pbdo_dt)(score_in, H, W, (double)(-w[0]), (double)(-w[1]), (double)(-w[2]), (double)(-w[3]),
                        m->anchors[d * 2 + 0], m->anchors[d * 2 + 1],
                        scoresp + HW * mm, Ixp + HW * mm, Iyp + HW * mm);
        }
        for (int pm = 0; pm < L; ++pm) { /* :134-160 */
            int *oIx = Ix + HW * (size_t)(slots[gp] + pm);
            int *oIy = Iy + HW * (size_t)(slots[gp] + pm);
            int *oIk = Ik + HW * (size_t)(slots[gp] + pm);
            const int fp = m->filterid[m->mix_offset[gpar] + pm];
            if (!nc[fp]) { /* :155 */
                nc[fp] = (REAL *)malloc(sizeof(REAL) * HW);
                memcpy(nc[fp], responses + (size_t)fp * HW, sizeof(REAL) * HW);
            }
            REAL *par = nc[fp];
            for (size_t i = 0; i < HW; ++i) {
                REAL v;
                int best;
                if (K == 1) { /* Math.hpp:153-158 */
                    v = scoresp[i] + (REAL)m->biasw[m->biasid[m->mix_offset[gp]] + pm];
                    best = 0;
                } else {
                    v = -(REAL)INFINITY;
                    best = 0;
                    for (int mm = 0; mm < K; ++mm) { /* :138-140 + Math.hpp:178-182 */
                        const REAL wv = scoresp[HW * mm + i] + (REAL)m->biasw[m->biasid[m->mix_offset[gp] + mm] + pm];
                        if (wv > v) { best = mm; v = wv; }
                    }
                }
                oIk[i] = best;
                oIx[i] = Ixp[HW * best + i];
                oIy[i] = Iyp[HW * best + i];
                par[i] += v; /* :156 */
            }
        }
        free(scoresp); free(Ixp); free(Iyp);
    }

    /* :163-171 root */
    {
        const int K = m->mix_offset[p0 + 1] - m->mix_offset[p0];
        const REAL bias = (REAL)m->biasw[m->biasid[m->mix_offset[p0]]];
        for (size_t i = 0; i < HW; ++i) {
            REAL v;
            int best = 0;
            if (K == 1) {
                const int f = m->filterid[m->mix_offset[p0]];
                v = (nc[f] ? nc[f][i] : responses[(size_t)f * HW + i]) + bias;
            } else {
                v = -(REAL)INFINITY;
                for (int mm = 0; mm < K; ++mm) {
                    const int f = m->filterid[m->mix_offset[p0] + mm];
                    /* a root without children never happens in the reference (empty Mat); use the raw response */
                    const REAL wv = (nc[f] ? nc[f][i] : responses[(size_t)f * HW + i]) + bias;
                    if (wv > v) { best = mm; v = wv; }
                }
            }
            rootv[i] = v;
            rooti[i] = best;
        }
    }
    for (int f = 0; f < m->nfilters; ++f) free(nc[f]);
    free(nc);
    free(slots);
}

/* ------------------------------------------------------------------------------------------
 * DynamicProgram<T>::argmin for one (level, component).  src/DynamicProgram.cpp:196-253.
 * ---------------------------------------------------------------------------------------- */
static inline int FN(round_mul)(int a, REAL s)
{ /* cv::Point_<int> * T -> saturate_cast<int>(a*s) = cvRound = round half to even */
    REAL p = (REAL)a * s;
    if (p >= (REAL)2147483647.0) return 2147483647;
    if (p <= (REAL)-2147483648.0) return (-2147483647 - 1);
    return (int)RINT_REAL(p);
}

int FN(pbdo_dp_argmin)(const pbdo_model *m, int c, int level, float scalef, int H, int W,
                       const int *Ix, const int *Iy, const int *Ik,
                       const REAL *rootv, const int *rooti,
                       pbdo_candidate_hdr *hdr, int *rects, int max_parts, int capacity)
{
    const size_t HW = (size_t)H * W;
    const int p0 = m->part_offset[c];
    const int nparts = m->part_offset[c + 1] - p0;
    const REAL scale = (REAL)scalef; /* :199 */
    int *slots = (int *)malloc(sizeof(int) * (size_t)m->part_offset[m->ncomponents]);
    pbdo_ptr_slots(m, slots);
    int *xv = (int *)malloc(sizeof(int) * nparts * 3), *yv = xv + nparts, *mv = yv + nparts;
    int count = 0;
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) { /* Math::find raster order, Math.hpp:84-93 */
            if (!(rootv[(size_t)y * W + x] > (REAL)m->thresh)) continue; /* :208 */
            if (count >= capacity || nparts > max_parts) { free(slots); free(xv); return -1; }
            pbdo_candidate_hdr *h = hdr + count;
            int *r = rects + (size_t)count * max_parts * 4;
            h->component = c; h->level = level; h->root_x = x; h->root_y = y;
            h->score = (float)rootv[(size_t)y * W + x]; h->nparts = nparts;
            for (int p = 0; p < nparts; ++p) { /* :218-244 */
                const int gp = p0 + p;
                if (p == 0) {
                    xv[0] = x; yv[0] = y; mv[0] = rooti[(size_t)y * W + x];
                } else {
                    const int idx = m->parentid[gp];
                    const int px = xv[idx], py = yv[idx], pm = mv[idx];
                    const size_t o = HW * (size_t)(slots[gp] + pm) + (size_t)py * W + px;
                    xv[p] = Ix[o]; yv[p] = Iy[o]; mv[p] = Ik[o];
                }
                const int ks = m->filter_ksize[m->filterid[m->mix_offset[gp] + mv[p]]]; /* xsize == ysize == rows */
                const int x1 = FN(round_mul)(xv[p] - 1, scale), y1 = FN(round_mul)(yv[p] - 1, scale);
                const int x2 = x1 + FN(round_mul)(ks, scale) - 1, y2 = y1 + FN(round_mul)(ks, scale) - 1;
                const int rx = x1 < x2 ? x1 : x2, ry = y1 < y2 ? y1 : y2;
                r[p * 4 + 0] = rx; r[p * 4 + 1] = ry;
                r[p * 4 + 2] = (x1 > x2 ? x1 : x2) - rx;
                r[p * 4 + 3] = (y1 > y2 ? y1 : y2) - ry;
            }
            ++count;
        }
    }
    free(slots);
    free(xv);
    return count;
}

/* ------------------------------------------------------------------------------------------
 * Staged helpers and the whole path.  src/PartsBasedDetector.cpp:69-95 with the reference's
 * five OpenMP sites (src/HOGFeatures.cpp:112,131; src/SpatialConvolutionEngine.cpp:115;
 * src/DynamicProgram.cpp:81,195).
 * ---------------------------------------------------------------------------------------- */
static const REAL *FN(model_filter)(const pbdo_model *m, int f)
{
    return FN(model_filters)(m) + m->filter_offset[f];
}

int FN(pbdo_features_d)(const pbdo_model *m, const void *im, int depth, int rows, int cols, int cn, size_t stride,
                        REAL *feat, int64_t *feat_offset, int *out_rows, int *out_cols, float *scales);
int FN(pbdo_features)(const pbdo_model *m, const uint8_t *im, int rows, int cols, int cn, size_t stride,
                      REAL *feat, int64_t *feat_offset, int *out_rows, int *out_cols, float *scales)
{
    return FN(pbdo_features_d)(m, im, PBDO_8U, rows, cols, cn, stride, feat, feat_offset, out_rows, out_cols, scales);
}

/* stride in elements of the image depth */
int FN(pbdo_features_d)(const pbdo_model *m, const void *im, int depth, int rows, int cols, int cn, size_t stride,
                        REAL *feat, int64_t *feat_offset, int *out_rows, int *out_cols, float *scales)
{
    const size_t es = pbdo_depth_size(depth);
    if (!es) return -3;
    int lr[PBDO_MAX_LEVELS], lc[PBDO_MAX_LEVELS];
    int64_t ioff[PBDO_MAX_LEVELS + 1];
    int n = pbdo_pyramid_plan(rows, cols, m->sbin, m->interval, lr, lc, scales);
    if (n <= 0) return n;
    size_t tot = 0;
    for (int l = 0; l < n; ++l) tot += (size_t)lr[l] * lc[l] * cn;
    char *imgs = (char *)malloc(tot * es);
    pbdo_pyramid_images(im, depth, rows, cols, cn, stride, m->sbin, m->interval, imgs, ioff, lr, lc, scales);
    int64_t off = 0;
    for (int l = 0; l < n; ++l) {
        pbdo_hog_dims(lr[l], lc[l], m->sbin, &out_rows[l], &out_cols[l]);
        feat_offset[l] = off;
        off += (int64_t)out_rows[l] * out_cols[l] * m->flen;
    }
    feat_offset[n] = off;
    if (feat) {
#pragma omp parallel for schedule(dynamic, 1)
        for (int l = 0; l < n; ++l) /* src/HOGFeatures.cpp:131-150 */
            FN(pbdo_hog_features_d)(imgs + ioff[l] * es, depth, lr[l], lc[l], cn, (size_t)lc[l] * cn, m->sbin, m->norient,
                                    m->flen, feat + feat_offset[l]);
    }
    free(imgs);
    return n;
}

void FN(pbdo_responses)(const pbdo_model *m, const REAL *feat, int H, int W, REAL *resp)
{
#pragma omp parallel for schedule(dynamic, 1)
    for (int f = 0; f < m->nfilters; ++f)
        FN(pbdo_conv)(feat, H, W, m->flen, FN(model_filter)(m, f), m->filter_ksize[f], resp + (size_t)f * H * W);
}

static int FN(cand_less)(const pbdo_candidate_hdr *a, const pbdo_candidate_hdr *b)
{
    if (a->level != b->level) return a->level < b->level;
    if (a->component != b->component) return a->component < b->component;
    if (a->root_y != b->root_y) return a->root_y < b->root_y;
    return a->root_x < b->root_x;
}

int FN(pbdo_detect_d)(const pbdo_model *m, const void *im, int depth, int rows, int cols, int cn, size_t stride,
                      pbdo_candidate_hdr *hdr, int *rects, int max_parts, int capacity, double *stage_ms);
int FN(pbdo_detect)(const pbdo_model *m, const uint8_t *im, int rows, int cols, int cn, size_t stride,
                    pbdo_candidate_hdr *hdr, int *rects, int max_parts, int capacity, double *stage_ms)
{
    return FN(pbdo_detect_d)(m, im, PBDO_8U, rows, cols, cn, stride, hdr, rects, max_parts, capacity, stage_ms);
}

/* stride in elements of the image depth */
int FN(pbdo_detect_d)(const pbdo_model *m, const void *im, int depth, int rows, int cols, int cn, size_t stride,
                      pbdo_candidate_hdr *hdr, int *rects, int max_parts, int capacity, double *stage_ms)
{
    const size_t es = pbdo_depth_size(depth);
    if (!es) return -3;
    int lr[PBDO_MAX_LEVELS], lc[PBDO_MAX_LEVELS], oh[PBDO_MAX_LEVELS], ow[PBDO_MAX_LEVELS];
    int64_t ioff[PBDO_MAX_LEVELS + 1], foff[PBDO_MAX_LEVELS + 1], roff[PBDO_MAX_LEVELS + 1];
    float scales[PBDO_MAX_LEVELS];
    double t0 = now_ms(), t1;
    int n = pbdo_pyramid_plan(rows, cols, m->sbin, m->interval, lr, lc, scales);
    if (n <= 0) return -2;

    /* features_->pyramid : images */
    size_t tot = 0;
    for (int l = 0; l < n; ++l) tot += (size_t)lr[l] * lc[l] * cn;
    char *imgs = (char *)malloc(tot * es);
    pbdo_pyramid_images(im, depth, rows, cols, cn, stride, m->sbin, m->interval, imgs, ioff, lr, lc, scales);
    t1 = now_ms(); if (stage_ms) stage_ms[0] = t1 - t0; t0 = t1;

    /* features_->pyramid : HOG */
    int64_t fo = 0, ro = 0;
    for (int l = 0; l < n; ++l) {
        pbdo_hog_dims(lr[l], lc[l], m->sbin, &oh[l], &ow[l]);
        foff[l] = fo; fo += (int64_t)oh[l] * ow[l] * m->flen;
        roff[l] = ro; ro += (int64_t)oh[l] * ow[l];
    }
    foff[n] = fo; roff[n] = ro;
    REAL *feat = (REAL *)malloc(sizeof(REAL) * (size_t)(fo > 0 ? fo : 1));
#pragma omp parallel for schedule(dynamic, 1)
    for (int l = 0; l < n; ++l)
        FN(pbdo_hog_features_d)(imgs + ioff[l] * es, depth, lr[l], lc[l], cn, (size_t)lc[l] * cn, m->sbin, m->norient, m->flen,
                                feat + foff[l]);
    free(imgs);
    t1 = now_ms(); if (stage_ms) stage_ms[1] = t1 - t0; t0 = t1;

    /* convolution_engine_->pdf: responses[level][filter]; level l's maps at resp + roff[l]*nfilters */
    REAL *resp = (REAL *)malloc(sizeof(REAL) * (size_t)(ro > 0 ? ro : 1) * m->nfilters);
#pragma omp parallel for schedule(dynamic, 1)
    for (int f = 0; f < m->nfilters; ++f) /* src/SpatialConvolutionEngine.cpp:115-123 */
        for (int l = 0; l < n; ++l)
            if (oh[l] > 0 && ow[l] > 0)
                FN(pbdo_conv)(feat + foff[l], oh[l], ow[l], m->flen, FN(model_filter)(m, f), m->filter_ksize[f],
                              resp + (size_t)roff[l] * m->nfilters + (size_t)f * oh[l] * ow[l]);
    free(feat);
    t1 = now_ms(); if (stage_ms) stage_ms[2] = t1 - t0; t0 = t1;

    /* dp_.min */
    const int totparts = m->part_offset[m->ncomponents];
    int *slots = (int *)malloc(sizeof(int) * (size_t)totparts);
    const int nslots = pbdo_ptr_slots(m, slots);
    const int C = m->ncomponents;
    int *Ix = (int *)malloc(sizeof(int) * (size_t)(ro > 0 ? ro : 1) * (nslots > 0 ? nslots : 1));
    int *Iy = (int *)malloc(sizeof(int) * (size_t)(ro > 0 ? ro : 1) * (nslots > 0 ? nslots : 1));
    int *Ik = (int *)malloc(sizeof(int) * (size_t)(ro > 0 ? ro : 1) * (nslots > 0 ? nslots : 1));
    REAL *rootv = (REAL *)malloc(sizeof(REAL) * (size_t)(ro > 0 ? ro : 1) * C);
    int *rooti = (int *)malloc(sizeof(int) * (size_t)(ro > 0 ? ro : 1) * C);
#pragma omp parallel for schedule(dynamic, 1)
    for (int nc = 0; nc < n * C; ++nc) { /* src/DynamicProgram.cpp:81-83 */
        const int l = nc / C, c = nc % C;
        if (oh[l] <= 0 || ow[l] <= 0) continue;
        FN(pbdo_dp_min)(m, c, resp + (size_t)roff[l] * m->nfilters, oh[l], ow[l],
                        Ix + (size_t)roff[l] * nslots, Iy + (size_t)roff[l] * nslots, Ik + (size_t)roff[l] * nslots,
                        rootv + (size_t)roff[l] * C + (size_t)c * oh[l] * ow[l],
                        rooti + (size_t)roff[l] * C + (size_t)c * oh[l] * ow[l]);
    }
    free(resp);
    t1 = now_ms(); if (stage_ms) stage_ms[3] = t1 - t0; t0 = t1;

    /* dp_.argmin; the reference pushes under omp critical in nondeterministic order, so levels are
     * walked serially here (negligible cost) and the list is sorted by (level, component, y, x). */
    int count = 0, overflow = 0;
    for (int l = 0; l < n && !overflow; ++l) {
        for (int c = 0; c < C; ++c) {
            if (oh[l] <= 0 || ow[l] <= 0) continue;
            int got = FN(pbdo_dp_argmin)(m, c, l, scales[l], oh[l], ow[l],
                                         Ix + (size_t)roff[l] * nslots, Iy + (size_t)roff[l] * nslots,
                                         Ik + (size_t)roff[l] * nslots,
                                         rootv + (size_t)roff[l] * C + (size_t)c * oh[l] * ow[l],
                                         rooti + (size_t)roff[l] * C + (size_t)c * oh[l] * ow[l],
                                         hdr + count, rects + (size_t)count * max_parts * 4, max_parts,
                                         capacity - count);
            if (got < 0) { overflow = 1; break; }
            count += got;
        }
    }
    (void)FN(cand_less); /* walk order above is already (level, component, y, x) */
    free(Ix); free(Iy); free(Ik); free(rootv); free(rooti); free(slots);
    t1 = now_ms(); if (stage_ms) stage_ms[4] = t1 - t0;
    return overflow ? -1 : count;
}
