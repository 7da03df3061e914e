// mask_rbox_body.inc -- the kernel bodies that both forms of the rotated box run, included as text inside a kernel so that the
// kernels of mask_rbox.hip stay token for token what they were (needs mask_rbox_common.h and `const RboxParams p` in scope):
//   RBOX_BODY_UNION : the links of word q of row y (y >= 1) to row y-1 of stream b (b, y, q: ints in scope)
//   RBOX_BODY_TRACE : the serial trace of stream RBOX_STREAM, one lane per root run (template parameter IN_LDS in scope)
//   RBOX_BODY_HULL  : hull, calipers and the output row of stream RBOX_STREAM from the rows [RBOX_Y0, RBOX_Y1) -- every row of the
//                     winner lies in that range, and rows without winner pixels never enter the chains, so the range changes no
//                     vertex and no order
#if defined(RBOX_BODY_UNION)
    const u64 *C = p.bits + ((size_t)b * p.H + y) * p.Wq, *A = C - p.Wq;
    const u64 c = C[q], a = A[q];
    if (!c) return;
    const u64 cl = shl1(C, q), cr = shr1(C, q, p.Wq), al = shl1(A, q), ar = shr1(A, q, p.Wq);
    u64 V = c & a & ~(cl & al);                         // straight up, unless column x-1 links the same two runs
    u64 DL = c & al & ~a & ~cl;                         // up-left, unless (x, y-1) or (x-1, y) makes the link
    u64 DR = c & ar & ~a & ~cr;                         // up-right likewise
    int *parent = p.parent + (size_t)b * p.H * p.Wh;
    int *err = &p.hdr[b].err;
    const int cap = p.H * p.Wh;
    while (V) {
        const int x = q * 64 + __ffsll((long long)V) - 1;
        V &= V - 1;
        uf_union(parent, y * p.Wh + (run_start(C, x) >> 1), (y - 1) * p.Wh + (run_start(A, x) >> 1), cap, err);
    }
    while (DL) {                                        // (x, y) starts its run
        const int x = q * 64 + __ffsll((long long)DL) - 1;
        DL &= DL - 1;
        uf_union(parent, y * p.Wh + (x >> 1), (y - 1) * p.Wh + (run_start(A, x - 1) >> 1), cap, err);
    }
    while (DR) {                                        // (x+1, y-1) starts its run
        const int x = q * 64 + __ffsll((long long)DR) - 1;
        DR &= DR - 1;
        uf_union(parent, y * p.Wh + (run_start(C, x) >> 1), (y - 1) * p.Wh + ((x + 1) >> 1), cap, err);
    }
#elif defined(RBOX_BODY_TRACE)
    extern __shared__ unsigned s_frame[];               // IN_LDS: [H + 2][2 Wq + 2] words, see LdsFrame
    __shared__ u64 s_best;
    __shared__ int s_ncomp, s_err;
    const int b = RBOX_STREAM, nwords = p.H * p.Wq, pitch = 2 * p.Wq + 2;
    const u64 *gbits = p.bits + (size_t)b * nwords;
    if (threadIdx.x == 0) { s_best = 0; s_ncomp = 0; s_err = 0; }
    if (IN_LDS) {
        for (int i = threadIdx.x; i < (p.H + 2) * pitch; i += blockDim.x) {
            const int y = i / pitch - 1, c = i - (y + 1) * pitch - 1;       // c: 32-bit word of row y, -1 and 2 Wq are the pads
            unsigned v = 0;
            if (y >= 0 && y < p.H && c >= 0 && c < 2 * p.Wq) v = (unsigned)(gbits[y * p.Wq + (c >> 1)] >> (32 * (c & 1)));
            s_frame[i] = v;
        }
    }
    __syncthreads();
    const int *parent = p.parent + (size_t)b * p.H * p.Wh;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < nwords; idx += gridDim.x * blockDim.x) {
        const int y = idx / p.Wq, q = idx - y * p.Wq;
        u64 starts = gbits[idx] & ~shl1(gbits + (size_t)y * p.Wq, q);
        while (starts) {
            const int x = q * 64 + __ffsll((long long)starts) - 1;
            starts &= starts - 1;
            const int slot = y * p.Wh + (x >> 1);
            if (parent[slot] != slot) continue;
            const long long a2 = IN_LDS ? trace_area2(LdsFrame{s_frame, pitch}, x, y, p.W, p.H)
                                        : trace_area2(GlobalFrame{gbits, p.H, p.Wq}, x, y, p.W, p.H);
            if (a2 < 0) { atomicOr(&s_err, 1); continue; }
            atomicAdd(&s_ncomp, 1);
            // larger area first, then the earlier first pixel; + 1 so that a component of area 0 still beats "none"
            atomicMax(&s_best, ((u64)a2 << 24 | (u64)(0xffffff - slot)) + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_ncomp) { atomicAdd(&p.hdr[b].ncomp, s_ncomp); atomicMax(&p.hdr[b].best, s_best); }
        if (s_err) atomicOr(&p.hdr[b].err, 1);
    }
#elif defined(RBOX_BODY_HULL)
    __shared__ unsigned s_row[RBOX_MAX_H];              // xmin | xmax << 16, ~0 for a row without winner pixels
    __shared__ unsigned s_chain[2][RBOX_MAX_H];         // the left chain and the right chain (x negated), both top to bottom
    __shared__ int s_n[2];
    __shared__ double s_area[RBOX_HULL_T];
    __shared__ int s_edge[RBOX_HULL_T];
    const int b = RBOX_STREAM, t = threadIdx.x;
    double *out = p.out + (size_t)b * 12;
    const RboxHdr hdr = p.hdr[b];
    if (hdr.err || !hdr.best) {                         // (block-uniform)
        if (t < 12) out[t] = t == 9 && hdr.err ? -1.0 : 0.0;
        return;
    }
    for (int y = RBOX_Y0 + t; y < RBOX_Y1; y += RBOX_HULL_T) {
        const int lo = p.rows[((size_t)b * p.H + y) * 2], hi = p.rows[((size_t)b * p.H + y) * 2 + 1];
        s_row[y] = hi < 0 ? ~0u : (unsigned)lo | (unsigned)hi << 16;
    }
    __syncthreads();
    if (t < 2) {                                        // lane 0: leftmost chain; lane 1: the same on the mirrored x = -xmax
        unsigned *st = s_chain[t];
        int n = 0;
        for (int y = RBOX_Y0; y < RBOX_Y1; ++y) {
            const unsigned r = s_row[y];
            if (r == ~0u) continue;
            const int x = t ? -(int)(r >> 16) : (int)(r & 0xffff);
            while (n >= 2) {                            // (pops <= pushes <= H)
                const int ax = ch_x(st[n - 2]), ay = ch_y(st[n - 2]), bx = ch_x(st[n - 1]), by = ch_y(st[n - 1]);
                if ((bx - ax) * (y - ay) - (by - ay) * (x - ax) < 0) break;    // strictly convex: keep
                --n;
            }
            st[n++] = ((unsigned)x & 0xffff) | (unsigned)y << 16;
        }
        s_n[t] = n;
    }
    __syncthreads();
    // the hull, cyclic: the left chain downwards, then the right chain upwards without the ends it shares with the left one
    const int nl = s_n[0];
    int nr = s_n[1], r_last = nr - 1;
    if (nl && nr && ch_x(s_chain[1][r_last]) == -ch_x(s_chain[0][nl - 1])) { --r_last; --nr; }   // bottom row of one pixel
    if (nl && nr && ch_x(s_chain[1][0]) == -ch_x(s_chain[0][0])) --nr;                            // top row of one pixel
    const int n = nl + nr;
    if (n == 0) {                                       // a winner without pixels: cannot happen; reported, not trusted
        if (t < 12) out[t] = t == 9 ? -1.0 : 0.0;
        return;
    }
    auto hx = [&](int i) { return i < nl ? ch_x(s_chain[0][i]) : -ch_x(s_chain[1][r_last - (i - nl)]); };
    auto hy = [&](int i) { return i < nl ? ch_y(s_chain[0][i]) : ch_y(s_chain[1][r_last - (i - nl)]); };
    // rotating calipers: every hull edge is a candidate side; extents as exact integers in units of the edge length
    double best = 1e300;
    int best_i = 0x7fffffff;
    long long bu0 = 0, bu1 = 0, bv0 = 0, bv1 = 0;
    int bex = 1, bey = 0;
    for (int i = t; i < (n >= 2 ? n : 0); i += RBOX_HULL_T) {
        const int j = i + 1 < n ? i + 1 : 0;
        const int ex = hx(j) - hx(i), ey = hy(j) - hy(i);
        int u0 = 0x7fffffff, u1 = -0x7fffffff, v0 = 0x7fffffff, v1 = -0x7fffffff;
        for (int k = 0; k < n; ++k) {
            const int x = hx(k), y = hy(k);
            const int u = x * ex + y * ey, v = y * ex - x * ey;
            u0 = min(u0, u); u1 = max(u1, u); v0 = min(v0, v); v1 = max(v1, v);
        }
        const double a = (double)((long long)(u1 - u0) * (long long)(v1 - v0)) / (double)(ex * ex + ey * ey);
        if (a < best) { best = a; best_i = i; bu0 = u0; bu1 = u1; bv0 = v0; bv1 = v1; bex = ex; bey = ey; }
    }
    s_area[t] = best; s_edge[t] = best_i;
    __syncthreads();
    for (int s = RBOX_HULL_T / 2; s > 0; s >>= 1) {
        if (t < s && (s_area[t + s] < s_area[t] || (s_area[t + s] == s_area[t] && s_edge[t + s] < s_edge[t]))) {
            s_area[t] = s_area[t + s]; s_edge[t] = s_edge[t + s];
        }
        __syncthreads();
    }
    if (n == 1) {
        if (t < 8) out[t] = (t & 1) ? (double)hy(0) : (double)hx(0);
    } else if (best_i == s_edge[0]) {                   // the thread that holds the winning edge (edge indices are unique)
        const double l2 = (double)(bex * bex + bey * bey);
        const long long us[4] = {bu0, bu1, bu1, bu0}, vs[4] = {bv0, bv0, bv1, bv1};
        for (int c = 0; c < 4; ++c) {                   // corner = (u e + v e_perp) / |e|^2, the numerators exact
            out[2 * c] = (double)(us[c] * bex - vs[c] * bey) / l2;
            out[2 * c + 1] = (double)(us[c] * bey + vs[c] * bex) / l2;
        }
    }
    if (t == 0) {
        const double area = 0.5 * (double)((hdr.best - 1) >> 24);
        out[8] = area;
        out[9] = area > p.min_area ? 1.0 : 0.0;
        out[10] = (double)hdr.ncomp;
        out[11] = (double)n;
    }
#endif
