// The gradient of the boundary search (included by mobo.hip, inside namespace aligner): what a training step needs
// behind log_alpha / gamma.  Build-defined like the search itself (oracle/mobo_oracle.py::boundary_search_backward,
// pinned there to autograd over a float64 torch restatement of the forward pass).
//
// With u_i(k) = la_{i-1}(k) - L_i(k) and q_i(j) = e_i(j) - la_i(j) the posterior of the previous boundary is
// r_i(k | j) = exp(u_i(k) + q_i(j)), and for a direct cotangent G_i(j) = dl/dla_i(j) the total derivative
// Z_i(j) = dl/dla_i(j) follows the adjoint of the alpha recursion, token rows from the last to the first:
//     Y_i(k)  = sum_{j in (k, k+D]} Z_i(j) r_i(k | j)          (what reaches row i through position k)
//     Z_{i-1} = G_{i-1} + Y_i,           Z_{I-1} = G_{I-1}
//     dl/de[i, m-1] = Z_i(m) - sum_{k in [m-D, m)} exp(e_i(m) - L_i(k)) Y_i(k)
// (the chain is locally normalised: the classical beta variable is identically one, gamma needs no backward pass).
// A cotangent on gamma enters G as alpha_i(j) * sum_{y >= j} (Gamma_{i+1}(y) - Gamma_i(y)).
//
// Launches:  mobo_norm_kernel (L, ring refill) -> with a gamma cotangent mobo_bwd_cotangent_kernel (G, whole chip)
//            -> mobo_bwd_chain_one_kernel / mobo_bwd_chain_kernel (the dependent chain over the token rows: Y)
//            -> mobo_bwd_grad_kernel (whole chip).
// The chain is the forward chain's mirror image: a row looks AHEAD at most D positions, so the position segments of
// an utterance hand their FIRST D entries of (Z, q) to the segment on their left through the ring, the rightmost
// segment runs ahead, and block index 0 of an utterance is its rightmost segment.

struct MoboBwdParams {
    const void *e;                    // [B,Tx,Ty] energies, as given to the search
    const int *t_xs, *t_ys;
    const float *log_alpha;           // [B,Tx,Ty] the search's output
    const float *g_la, *g_ga;         // nullable cotangents [B,Tx,Ty]
    float *grad;                      // [B,Tx,Ty] out
    float *Lw;                        // workspace [B,Tx,Ty]: L_i(k), base 2
    const float *G;                   // G_i(j) at [i, j-1]: g_la itself, or the workspace plane the cotangent kernel wrote
    float *Gw;                        // workspace [B,Tx,Ty] (used with a gamma cotangent)
    float *Yw;                        // workspace [B,Tx,Ty]: Y_i(k); written by the chain wherever L_i(k) is live
    unsigned *ring;                   // workspace [B,S-1,Tx,2,D]: (Z, q) of a segment's first D positions, row by row
    int *failw;
    unsigned *trash;
    int *status;
    int B, Tx, Ty, D, S, nmax, start_lag, drop_seg, spin_limit;
    unsigned long long *stamps;       // development (aligner_debug_set_stamps): per block 24 words of phase cycle totals
    int stamp_wave;                   // ... taken by the first lane of this wave
};

constexpr float MB_FINITE = -3e38f;               // a log-probability above this is "not log 0" (-inf fails the test)

// ---------------------------------------------------------------------------------------------------------
// the direct cotangent with a gamma term: G_i(j) = g_la + alpha_i(j) sum_{y >= j} (Gamma_{i+1}(y) - Gamma_i(y)).
// One workgroup per (utterance, token row), frames from the right (a suffix sum).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mobo_bwd_cotangent_kernel(MoboBwdParams p) {
    __shared__ float wsum[4];
    __shared__ float s_carry;
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int I = p.t_xs[b], J = p.t_ys[b];
    I = I > p.Tx ? p.Tx : I;
    J = J > p.Ty ? p.Ty : J;
    if (i >= I || I < 1 || J < I) return;             // (rows nobody reads)
    const size_t ro = ((size_t)b * p.Tx + i) * p.Ty;
    if (tid == 0) s_carry = 0.f;
    __syncthreads();
    for (int y0 = (J - 1) / 256 * 256; y0 >= 0; y0 -= 256) {
        const int y = y0 + 255 - tid;                     // thread order = frames from the right
        const bool in = y < J;
        float dg = 0.f;
        if (in) dg = ((i + 1 < I) ? p.g_ga[ro + p.Ty + y] : 0.f) - p.g_ga[ro + y];
        float s = dg;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float t = __shfl_up(s, off);
            if (lane >= off) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        float base = s_carry;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        const float excl = base + s - dg;                 // sum over frames y' > y, i.e. y' >= j = y + 1
        __syncthreads();
        if (tid == 255) s_carry = base + s;
        __syncthreads();
        if (in) {
            const float la = p.log_alpha[ro + y];
            float g = 0.f;
            if (la > MB_FINITE) g = (p.g_la ? p.g_la[ro + y] : 0.f) + __expf(la) * excl;
            p.Gw[ro + y] = g;
        }
    }
}

// u_i(k), q_i(j), Z_i(j) of ONE boundary position x (as j in row i, as k out of row i-1), base 2
struct MbBwdCell {
    float z, q, u;
    bool live_j, live_k;
};
__device__ __forceinline__ MbBwdCell mb_bwd_cell(int i, int x, int J, int lo, int hi, float ev, float la_i, float la_im1,
                                                 float L, float g, float y_above) {
    MbBwdCell c;
    c.live_j = x >= 1 && x >= lo && x <= hi && la_i > MB_FINITE && ev > MB_FINITE && ev < -MB_FINITE;
    c.q = c.live_j ? (ev - la_i) * MB_LOG2E : MB_NEG;
    c.z = c.live_j ? g + y_above : 0.f;
    const float lap = (i == 0) ? (x == 0 ? 0.f : -__builtin_huge_valf()) : (x >= 1 ? la_im1 : -__builtin_huge_valf());
    c.live_k = x < J && L > MB_DEADF && lap > MB_FINITE;
    c.u = c.live_k ? lap * MB_LOG2E - L : MB_NEG;
    return c;
}

// ---------------------------------------------------------------------------------------------------------
// the chain, general form: any number of positions per thread, every window term its own exp2 (no reference,
// no range to watch).  Z of a position lives in a register (!MULTI) or in LDS (MULTI).
// LDS: two buffers (row parity) of (Z, q) for the segment's positions FOLLOWED by the D halo entries of the
// segment on the right.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mb_clean_bits(float z) {           // a value is never the ring's filler
    const unsigned w = __builtin_bit_cast(unsigned, z);
    return w == MB_FILL ? 0x7FC00000u : w;
}

struct MbBwdSeg {                       // a block's segment of its utterance (the mirror of the forward's numbering)
    int I, J, a, bnd, nloc, sg, Sne;
    bool valid, has_src, has_dst;
};
__device__ __forceinline__ MbBwdSeg mb_bwd_segment(const MoboBwdParams &p, int b, int sr) {
    MbBwdSeg g;
    g.valid = mb_lengths(p.t_xs, p.t_ys, p.Tx, p.Ty, p.D, b, g.I, g.J);
    g.a = g.bnd = g.nloc = g.sg = g.Sne = 0;
    g.has_src = g.has_dst = false;
    if (!g.valid) return g;
    const int P = g.J + 1;
    int Sb, n;
    mb_cut(g.J, p.D, p.S, Sb, n);
    g.Sne = (P + n - 1) / n;                       // segments that hold a position
    if (sr >= g.Sne) {
        g.valid = false;
        return g;
    }
    g.sg = g.Sne - 1 - sr;                         // block 0 of an utterance is its RIGHTMOST segment
    g.a = g.sg * n;
    g.bnd = (g.a + n < P) ? g.a + n : P;
    g.nloc = g.bnd - g.a;
    g.has_src = g.sg + 1 < g.Sne;
    g.has_dst = g.sg > 0 && g.sg != p.drop_seg;
    return g;
}
template <int VT, bool MULTI>
__global__ __launch_bounds__(1024) void mobo_bwd_chain_kernel(MoboBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, T = blockDim.x;
    const int b = blockIdx.x / p.S, sr = blockIdx.x - b * p.S;
    const int D = p.D;
    const MbBwdSeg g = mb_bwd_segment(p, b, sr);
    if (!g.valid) {
        if (sr == 0 && tid == 0 && g.Sne == 0) atomicOr(p.status, ALIGNER_ST_BAD_LENGTHS);
        return;
    }
    const int I = g.I, J = g.J, a = g.a, bnd = g.bnd, nloc = g.nloc;
    const int W = p.nmax + D;
    float *sZ = reinterpret_cast<float *>(smem);
    float *sQ = sZ + 2 * W;
    float *sY = sQ + 2 * W;                              // MULTI: Y of the row above, per position
    for (int h = tid; h < D; h += T) {                   // beyond the utterance's end (the rightmost segment keeps these)
        sZ[nloc + h] = 0.f;       sZ[W + nloc + h] = 0.f;
        sQ[nloc + h] = MB_NEG;    sQ[W + nloc + h] = MB_NEG;
    }
    if (MULTI)
        for (int x = tid; x < nloc; x += T) sY[x] = 0.f;
    float Yreg = 0.f;
    const size_t ubase = (size_t)b * p.Tx * p.Ty;
    unsigned *ring_out = p.ring + ((size_t)b * (p.S - 1) + (g.has_dst ? g.sg - 1 : 0)) * (size_t)p.Tx * 2 * D;
    const unsigned *ring_in = p.ring + ((size_t)b * (p.S - 1) + (g.has_src ? g.sg : 0)) * (size_t)p.Tx * 2 * D;
    int i0, i1;
    mb_active_rows(I, J, D, a, bnd, i0, i1);
    const int itop = (i1 < 0) ? -1 : (i1 + 1 < I ? i1 + 1 : I - 1);
    bool gave_up = false;
    __syncthreads();
    for (int i = I - 1; i >= 0; --i) {
        const bool active = i1 >= 0 && i >= i0 && i <= itop;
        if (!active) {                                   // nothing of this row lives here: "0 mass, log 0" to the left
            if (g.has_dst)
                for (int h = tid; h < D; h += T) {
                    unsigned *r = ring_out + (size_t)i * 2 * D + h;
                    mb_ring_store(r, 0u);
                    mb_ring_store(r + D, __builtin_bit_cast(unsigned, MB_NEG));
                }
            continue;
        }
        const size_t ro = ubase + (size_t)i * p.Ty;
        const int bo = (i & 1) * W;
        int lo, hi;
        mb_bounds(I, J, D, i, lo, hi);
        // ---- phase 1: Z_i(j) = G_i(j) + Y_{i+1}(j) and q_i(j) of the segment's own positions ----
#pragma unroll 1
        for (int x = tid; x < nloc; x += T) {
            const int j = a + x;
            float z = 0.f, q = MB_NEG;
            if (j >= 1) {
                const MbBwdCell c = mb_bwd_cell(i, j, J, lo, hi, mb_value<VT>(mb_load_raw<VT>(p.e, ro + (j - 1))),
                                                p.log_alpha[ro + (j - 1)], 0.f, MB_NEG, p.G[ro + (j - 1)], MULTI ? sY[x] : Yreg);
                z = c.z;
                q = c.q;
            }
            sZ[bo + x] = z;
            sQ[bo + x] = q;
            if (g.has_dst && x < D) {
                unsigned *r = ring_out + (size_t)i * 2 * D + x;
                mb_ring_store(r, mb_clean_bits(z));
                mb_ring_store(r + D, __builtin_bit_cast(unsigned, q));
            }
            if (!MULTI) break;
        }
        if (g.has_dst)                                   // (a last segment shorter than the window)
            for (int h = nloc + tid; h < D; h += T) {
                unsigned *r = ring_out + (size_t)i * 2 * D + h;
                mb_ring_store(r, 0u);
                mb_ring_store(r + D, __builtin_bit_cast(unsigned, MB_NEG));
            }
        // ---- the D entries after the segment: row i of the segment on the right ----
        if (g.has_src) {
#pragma unroll 1
            for (int h = tid; h < D; h += T) {
                const unsigned *r = ring_in + (size_t)i * 2 * D + h;
                unsigned w0 = mb_ring_load(r), w1 = mb_ring_load(r + D);
                int spins = 0;
                while ((w0 == MB_FILL || w1 == MB_FILL) && !gave_up) {
                    __builtin_amdgcn_s_sleep(4);
                    w0 = mb_ring_load(r);
                    w1 = mb_ring_load(r + D);
                    if (++spins > p.spin_limit) gave_up = true;
                }
                const bool bad = (w0 == MB_FILL || w1 == MB_FILL);
                sZ[bo + nloc + h] = bad ? 0.f : __builtin_bit_cast(float, w0);
                sQ[bo + nloc + h] = bad ? MB_NEG : __builtin_bit_cast(float, w1);
            }
        }
        lds_barrier();
        // ---- phase 2: Y_i(k) = sum_{j in (k, k+D]} Z_i(j) 2^(u_i(k) + q_i(j)) ----
#pragma unroll 1
        for (int x = tid; x < nloc; x += T) {
            const int k = a + x;
            float y = 0.f;
            if (k < J) {
                const MbBwdCell c = mb_bwd_cell(i, k, J, lo, hi, 0.f, 0.f, (i > 0 && k >= 1) ? p.log_alpha[ro - p.Ty + (k - 1)] : 0.f,
                                                p.Lw[ro + k], 0.f, 0.f);
                const float u = c.u;
                if (c.live_k) {
                    const float *z = sZ + bo + x + 1, *q = sQ + bo + x + 1;
                    float acc0 = 0.f, acc1 = 0.f;
                    int c = 0;
                    for (; c + 2 <= D; c += 2) {
                        acc0 += z[c] * __builtin_amdgcn_exp2f(u + q[c]);
                        acc1 += z[c + 1] * __builtin_amdgcn_exp2f(u + q[c + 1]);
                    }
                    if (c < D) acc0 += z[c] * __builtin_amdgcn_exp2f(u + q[c]);
                    y = acc0 + acc1;
                }
                p.Yw[ro + k] = y;
            }
            if (MULTI) sY[x] = y;
            else Yreg = y;
            if (!MULTI) break;
        }
    }
    if (gave_up) {
        atomicOr(p.status, ALIGNER_ST_INTERNAL);
        p.failw[b] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// the chain, split form (at most one position per H lanes): the mirror image of mobo_chain_one_kernel, with the same
// devices -- a straight-line row body (every lane issues every load and store of a row, lanes with nothing to say
// address the trash area, so hipcc emits counted waits), a helper wave that fetches, awaits and stages the halo, H
// lanes per window meeting through DPP quad exchanges, and the FAST sum: every entry also leaves
// t = Z 2^(q + R) against an integer reference R common to the workgroup, so a window is D additions and
// Y = 2^(u - R) sum t; while every live -q and u of the row (halo included) lies within 100 of R nothing leaves the
// range of a float.  A row with an entry out of range takes one exp2 per term (exponent u + q <= 0).
// ---------------------------------------------------------------------------------------------------------
template <int VT, int H, bool STAMPS>
__global__ __launch_bounds__(1024) void mobo_bwd_chain_one_kernel(MoboBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const bool stamping = STAMPS && p.stamps != nullptr && tid == 64 * p.stamp_wave;      // (a build of its own: the stamps cost registers)
    unsigned long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_t = 0, st_entry = 0, st_rt = 0, st_slow = 0;
    if (stamping) { st_entry = __builtin_amdgcn_s_memtime(); st_rt = __builtin_amdgcn_s_memrealtime(); }
#define MB_STAMP(k_) if (stamping) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st_acc[k_] += t_ - st_t; st_t = t_; }
    const bool has_helper = p.S > 1;
    const int T = (int)blockDim.x - (has_helper ? 64 : 0);
    const bool helper = tid >= T;
    const int b = blockIdx.x / p.S, sr = blockIdx.x - b * p.S;
    const int D = p.D;
    const MbBwdSeg g = mb_bwd_segment(p, b, sr);
    if (!g.valid) {
        if (sr == 0 && tid == 0 && g.Sne == 0) atomicOr(p.status, ALIGNER_ST_BAD_LENGTHS);
        return;
    }
    const int I = g.I, J = g.J, a = g.a, bnd = g.bnd, nloc = g.nloc;
    const int W = p.nmax + D;
    float *sZ = reinterpret_cast<float *>(smem);
    float *sQ = sZ + 2 * W;
    float *sT = sQ + 2 * W;
    int *sRep = reinterpret_cast<int *>(sT + 2 * W);      // [row parity][16 waves][2]: the waves' reports (mb_report_put)
    float *sSpare = reinterpret_cast<float *>(sRep + 64);  // where lanes without a position write (never read)
    if (tid < 32) { sRep[2 * tid] = MB_DEADM; sRep[2 * tid + 1] = 0; }
    for (int h = tid; h < D; h += T) {                    // beyond the utterance's end (the rightmost segment keeps these)
        sZ[nloc + h] = 0.f;       sZ[W + nloc + h] = 0.f;
        sQ[nloc + h] = MB_NEG;    sQ[W + nloc + h] = MB_NEG;
        sT[nloc + h] = 0.f;       sT[W + nloc + h] = 0.f;
    }
    lds_barrier();
    const int pi = tid / H, sub = tid - pi * H;
    const int j1 = a + pi;
    const bool mine = !helper && j1 < bnd;
    const bool lead = mine && sub == 0;
    const size_t ubase = (size_t)b * p.Tx * p.Ty;
    unsigned *trash = p.trash + (size_t)blockIdx.x * 1024 + tid;
    unsigned *ring_out = p.ring + ((size_t)b * (p.S - 1) + (g.has_dst ? g.sg - 1 : 0)) * (size_t)p.Tx * 2 * D;
    const unsigned *ring_in = p.ring + ((size_t)b * (p.S - 1) + (g.has_src ? g.sg : 0)) * (size_t)p.Tx * 2 * D;
    const int hl = tid - T;
    const bool publishes = g.has_dst && !helper && sub == 0 && pi < D;     // (a lane past a short last segment: "log 0")
    const int w0 = (sub * D) / H, w1 = ((sub + 1) * D) / H;
    int i0, i1;
    mb_active_rows(I, J, D, a, bnd, i0, i1);
    auto dead_rows = [&](int from, int to) {             // rows from > ... > to without anything of this segment: "0 mass"
        if (g.has_dst && !helper)
            for (int i = from; i > to; --i)
                for (int h = tid; h < D; h += T) {
                    unsigned *r = ring_out + (size_t)i * 2 * D + h;
                    mb_ring_store(r, 0u);
                    mb_ring_store(r + D, __builtin_bit_cast(unsigned, MB_NEG));
                }
    };
    if (i1 < 0) {
        dead_rows(I - 1, -1);
        return;
    }
    const int itop = i1 + 1 < I ? i1 + 1 : I - 1;         // row i1+1 still draws on this segment's positions of row i1
    dead_rows(I - 1, itop);
    bool gave_up = false;
    int R = 0;
    const int wave = tid >> 6, lane = tid & 63;

    if (helper) {
        // ------------------------------ the helper wave: the halo of rows itop..i0 ------------------------------
        if (g.has_src) {
            if (p.start_lag > 0) {                        // let the segment on the right get `start_lag` rows ahead first
                int ig = itop - p.start_lag;
                ig = ig < 0 ? 0 : ig;
                const unsigned *r = ring_in + (size_t)ig * 2 * D + (hl < D ? hl : 0) + D;
                int spins = 0;
                while (mb_ring_load(r) == MB_FILL && !gave_up) {
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > p.spin_limit) gave_up = true;
                }
            }
            const bool fetches = hl < D;
            unsigned h0_nx, h1_nx;
            auto issue_halo = [&](int i) {
                const unsigned *r = fetches ? ring_in + (size_t)i * 2 * D + hl : trash;
                h0_nx = mb_ring_load(r);
                h1_nx = mb_ring_load(r + (fetches ? D : 0));
            };
            issue_halo(itop);
#pragma unroll 1
            for (int i = itop; i >= i0; --i) {
                const unsigned h_c0 = h0_nx, h_c1 = h1_nx;
                issue_halo(i > 0 ? i - 1 : 0);
                const int bo = (i & 1) * W + nloc;
                int Mstat = MB_DEADM;
                bool fits = true;
                auto halo_entry = [&](int h, unsigned x0, unsigned x1) {
                    if (x0 == MB_FILL || x1 == MB_FILL) {                  // not published yet: poll
                        const unsigned *r = ring_in + (size_t)i * 2 * D + h;
                        int spins = 0;
                        do {
                            __builtin_amdgcn_s_sleep(2);
                            x0 = mb_ring_load(r);
                            x1 = mb_ring_load(r + D);
                            if (++spins > p.spin_limit) gave_up = true;
                        } while ((x0 == MB_FILL || x1 == MB_FILL) && !gave_up);
                    }
                    const bool bad = (x0 == MB_FILL || x1 == MB_FILL);
                    const float z = bad ? 0.f : __builtin_bit_cast(float, x0);
                    const float q = bad ? MB_NEG : __builtin_bit_cast(float, x1);
                    sZ[bo + h] = z;
                    sQ[bo + h] = q;
                    sT[bo + h] = z * __builtin_amdgcn_exp2f(q + (float)R);
                    if (q > MB_DEADF) {
                        const int M = (int)ceilf(-q);
                        Mstat = M;
                        fits = fits && M >= R - 100 && M <= R + 100;
                    }
                };
                if (fetches) halo_entry(hl, h_c0, h_c1);
                if (D > 64) {
#pragma unroll 1
                    for (int h = hl + 64; h < D; h += 64) halo_entry(h, MB_FILL, MB_FILL);
                }
                {
                    const unsigned long long lm = __builtin_amdgcn_ballot_w64(Mstat != MB_DEADM);
                    const bool wfit = __builtin_amdgcn_ballot_w64(!fits) == 0;
                    const int wm = lm ? __builtin_amdgcn_readlane(Mstat, __builtin_ctzll(lm)) : MB_DEADM;
                    mb_report_put(sRep, i & 1, wave, wm, wfit ? 0 : 1);
                }
                lds_barrier();
                int Rn, slow;
                mb_report_get(sRep, i & 1, lane, Rn, slow);
                R = (Rn != MB_DEADM) ? Rn : R;
            }
        }                                                 // (no segment to the right: the wave ends, a barrier only counts live waves)
        if (gave_up) {
            atomicOr(p.status, ALIGNER_ST_INTERNAL);
            p.failw[b] = 1;
        }
        return;
    }

    // ------------------------------ the compute waves ------------------------------
    const int je = (j1 < 1 ? 1 : (j1 > J ? J : j1)) - 1;               // frame of this lane's boundary position
    const int kl = j1 > J - 1 ? J - 1 : j1;
    // The operands of a row are requested TWO rows ahead: they come from HBM (every row a new cache line per plane), and a
    // row (~2 500 cycles) is about one HBM round trip -- with one row of lead some wave of the workgroup found its
    // operands late in most rows and the others waited for it at the barrier (~500 cycles of every row, in every wave).
    // Two register sets take turns (the loop is unrolled by two): shifting a queue with moves would wait for the
    // younger set's loads, a move reads its source.
    unsigned e_n1, e_n2;
    float L_n1, g_n1, la_n1, L_n2, g_n2, la_n2;
    auto issue = [&](int i, unsigned &e_o, float &L_o, float &g_o, float &la_o) {   // row i: e_i, L_i, G_i, log_alpha of row i-1
        const size_t ro = ubase + (size_t)i * p.Ty;
        e_o = mb_load_raw<VT>(p.e, ro + je);
        L_o = p.Lw[ro + kl];
        g_o = p.G[ro + je];
        la_o = p.log_alpha[ro - (i > 0 ? p.Ty : 0) + je];
    };
    float la_i = p.log_alpha[ubase + (size_t)itop * p.Ty + je];
    float y_above = 0.f;                                               // Y_{i+1}(j1)
    // (the loop is entered in the state every later row finds -- two rows of loads with a row's three stores behind
    // each: see mobo_chain_one_kernel)
    issue(itop, e_n1, L_n1, g_n1, la_n1);
    mb_ring_store(trash, 0u);
    mb_ring_store(trash, 0u);
    mb_ring_store(trash, 0u);
    issue(itop > 0 ? itop - 1 : 0, e_n2, L_n2, g_n2, la_n2);
    mb_ring_store(trash, 0u);
    mb_ring_store(trash, 0u);
    mb_ring_store(trash, 0u);
    unsigned long long st_loop = 0, bw_acc = 0;
    if (stamping) { st_loop = st_t = __builtin_amdgcn_s_memtime(); }
    auto do_row = [&](const int i, unsigned &e_s, float &L_s, float &g_s, float &la_s) {
        int lo, hi;
        mb_bounds(I, J, D, i, lo, hi);
        const unsigned e_c = e_s;
        const float L_c = L_s, g_c = g_s, lam_c = la_s;
        issue(i > 1 ? i - 2 : 0, e_s, L_s, g_s, la_s);              // (the set just read takes the row after next)
        if (stamping) { asm volatile("" :: "v"(e_c), "v"(L_c), "v"(g_c), "v"(lam_c)); }
        MB_STAMP(0)
        const size_t ro = ubase + (size_t)i * p.Ty;
        const int bo = (i & 1) * W;
        const MbBwdCell c = mb_bwd_cell(i, mine ? j1 : -1, J, lo, hi, mb_value<VT>(e_c), la_i, lam_c, mine ? L_c : MB_NEG, g_c, y_above);
        // ---- phase 1: this position as the END of token i ----
        {
            // (no branch in here: every lane writes -- the lanes of a position the same words, lanes past the segment
            // a spare entry -- and the report is plain integer logic; a uniform branch costs ~20 cycles taken or not)
            const float tval = c.z * __builtin_amdgcn_exp2f(c.q + (float)R);
            float *wz = mine ? sZ + bo + pi : sSpare;
            wz[0] = c.z;
            (mine ? wz + 2 * W : wz + 1)[0] = c.q;
            (mine ? wz + 4 * W : wz + 2)[0] = tval;
            {   // the wave's report: "an entry does not fit" and ANY live exponent as the next row's reference
                const int Mq = (int)ceilf(-c.q), Mu = (int)ceilf(c.u);
                const unsigned dq = (unsigned)Mq - (unsigned)R + 100u, du = (unsigned)Mu - (unsigned)R + 100u;
                const int lq = (int)lead & (int)c.live_j, lu = (int)lead & (int)c.live_k;
                const int nofit = (lq & (int)(dq > 200u)) | (lu & (int)(du > 200u));
                const int Mc = lq ? Mq : Mu;
                const unsigned long long lm = __builtin_amdgcn_ballot_w64((lq | lu) != 0);
                const unsigned long long nf = __builtin_amdgcn_ballot_w64(nofit != 0);
                const int wm = lm ? __builtin_amdgcn_readlane(Mc, __builtin_ctzll(lm)) : MB_DEADM;
                mb_report_put(sRep, i & 1, wave, wm, nf ? 1 : 0);
            }
            unsigned *r = publishes ? ring_out + (size_t)i * 2 * D + pi : trash;
            mb_ring_store(r, mb_clean_bits(c.z));
            mb_ring_store(r + (publishes ? D : 0), __builtin_bit_cast(unsigned, c.q));
        }
        MB_STAMP(1)
        if (STAMPS) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
        MB_STAMP(5)
        unsigned long long bw_t = 0;
        if (STAMPS && p.stamps != nullptr) bw_t = __builtin_amdgcn_s_memtime();           // every wave: its own wait at the barrier
        lds_barrier();
        if (STAMPS && p.stamps != nullptr) {
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();
            bw_acc += t_ - bw_t;
            const int rr = itop - 20 - i;                                   // a trace of 16 rows, block 4 only
            if (blockIdx.x == 4 && lane == 0 && wave < 4 && rr >= 0 && rr < 16) {
                p.stamps[2048 * 24 + (rr * 4 + wave) * 2] = bw_t;
                p.stamps[2048 * 24 + (rr * 4 + wave) * 2 + 1] = t_;
            }
        }
        MB_STAMP(2)
        // ---- phase 2: this position as the START of token i: Y_i(k) over the window (k, k+D] ----
        {
            // the window's first 16 fast terms are requested before the report is looked at (LDS answers in order and a
            // lone wave per SIMD pays every round trip in full); entries past the lane's part are read and dropped
            const int x = bo + (mine ? pi : 0) + 1 + w0;
            const int cnt = w1 - w0;
            const float *t = sT + x;
            float tv[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) tv[k] = t[k];
            int Rn, slow;
            mb_report_get(sRep, i & 1, lane, Rn, slow);
            float acc;
            if (!slow) {
#pragma unroll
                for (int k = 0; k < 16; ++k) tv[k] = (k < cnt) ? tv[k] : 0.f;
                acc = (((tv[0] + tv[1]) + (tv[2] + tv[3])) + ((tv[4] + tv[5]) + (tv[6] + tv[7]))) +
                      (((tv[8] + tv[9]) + (tv[10] + tv[11])) + ((tv[12] + tv[13]) + (tv[14] + tv[15])));
#pragma unroll 1
                for (int c0 = 16; c0 < cnt; c0 += 16) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) tv[k] = t[c0 + k];
#pragma unroll
                    for (int k = 0; k < 16; ++k) tv[k] = (c0 + k < cnt) ? tv[k] : 0.f;
                    acc += (((tv[0] + tv[1]) + (tv[2] + tv[3])) + ((tv[4] + tv[5]) + (tv[6] + tv[7]))) +
                           (((tv[8] + tv[9]) + (tv[10] + tv[11])) + ((tv[12] + tv[13]) + (tv[14] + tv[15])));
                }
#pragma unroll
                for (int m = 1; m < H; m <<= 1) acc += mb_quad_xor_f(acc, m);
                acc *= __builtin_amdgcn_exp2f(c.u - (float)R);
            } else {
                if (stamping) ++st_slow;
                const float *z = sZ + x, *q = sQ + x;
                acc = 0.f;
#pragma unroll 1
                for (int c0 = 0; c0 < cnt; c0 += 8) {
                    float zv[8], qv[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) { zv[k] = z[c0 + k]; qv[k] = q[c0 + k]; }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float term = zv[k] * __builtin_amdgcn_exp2f(c.u + qv[k]);
                        acc += (c0 + k < cnt) ? term : 0.f;
                    }
                }
#pragma unroll
                for (int m = 1; m < H; m <<= 1) acc += mb_quad_xor_f(acc, m);
            }
            const float y = c.live_k ? acc : 0.f;
            y_above = y;
            la_i = lam_c;
            R = (Rn != MB_DEADM) ? Rn : R;
            if (stamping) { asm volatile("" :: "v"(y)); }
            MB_STAMP(3)
            float *yp = (lead && j1 < J) ? p.Yw + ro + j1 : reinterpret_cast<float *>(trash);
            *yp = y;
        }
        MB_STAMP(4)
    };
#pragma unroll 1
    for (int i = itop; i >= i0; i -= 2) {
        do_row(i, e_n1, L_n1, g_n1, la_n1);
        if (i - 1 < i0) break;
        do_row(i - 1, e_n2, L_n2, g_n2, la_n2);
    }
    if (STAMPS && p.stamps != nullptr && lane == 0 && wave < 8) p.stamps[(size_t)blockIdx.x * 24 + 15 + wave] = bw_acc;
    if (stamping) {
        unsigned long long *o = p.stamps + (size_t)blockIdx.x * 24;
        o[0] = st_entry; o[1] = st_loop; o[2] = __builtin_amdgcn_s_memtime();
        for (int q = 0; q < 6; ++q) o[3 + q] = st_acc[q];
        o[9] = (unsigned long long)(itop - i0 + 1); o[10] = (unsigned long long)i0; o[11] = st_rt;
        o[12] = __builtin_amdgcn_s_memrealtime(); o[13] = 0; o[14] = st_slow;
    }
#undef MB_STAMP
    dead_rows(i0 - 1, -1);
}

// ---------------------------------------------------------------------------------------------------------
// the gradient: dl/de[i, m-1] = Z_i(m) - 2^(e_i(m)) sum_{k in [m-D, m)} 2^(-L_i(k)) Y_i(k), every cell at once.
// grid (ceil(Ty/1024), Tx, B) x 256 threads, four frames per thread, the window's terms from LDS.
// ---------------------------------------------------------------------------------------------------------
template <int VT>
__global__ __launch_bounds__(256) void mobo_bwd_grad_kernel(MoboBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_ref;
    const int tid = threadIdx.x;
    const int b = blockIdx.z, i = blockIdx.y, y0 = blockIdx.x * MB_NCH;
    const int D = p.D;
    int I = p.t_xs[b], J = p.t_ys[b];
    I = I > p.Tx ? p.Tx : I;
    J = J > p.Ty ? p.Ty : J;
    bool ok = I >= 1 && J >= I && (long long)J <= (long long)I * D && !p.failw[b];
    // masked frames that leave P(b_{I-1} = J) = 0 leave no segmentation either: no gradient, as for such lengths
    ok = ok && p.log_alpha[((size_t)b * p.Tx + (I - 1)) * p.Ty + (J - 1)] > MB_FINITE;
    const size_t ro = ((size_t)b * p.Tx + i) * p.Ty;
    if (!ok || i >= I || y0 >= J) {
        for (int y = y0 + tid; y < y0 + MB_NCH && y < p.Ty; y += 256) p.grad[ro + y] = 0.f;
        return;
    }
    // staged entries x = 0 .. NE-1 stand for previous boundaries k = y0 + 1 - D + x  (frame y = m-1 needs k in [y+1-D, y])
    const int NE = MB_NCH + D - 1;
    float *sL = reinterpret_cast<float *>(smem);          // L_i(k), "log 0" where nothing flows
    float *sYv = sL + NE;                                 // Y_i(k)
    float *sC = sYv + NE;                                 // Y_i(k) 2^(Rb - L_i(k))
    if (tid == 0) s_ref = MB_DEADM;
    __syncthreads();
    int Lmax = MB_DEADM;
    for (int x = tid; x < NE; x += 256) {
        const int k = y0 + 1 - D + x;
        float L = MB_NEG, yv = 0.f;
        if (k >= 0 && k < J) {
            yv = p.Yw[ro + k];
            L = p.Lw[ro + k];
            if (!(L > MB_DEADF) || yv == 0.f) { L = MB_NEG; yv = 0.f; }
        }
        sL[x] = L;
        sYv[x] = yv;
        if (L > MB_DEADF) {
            const int M = (int)ceilf(L);
            Lmax = Lmax > M ? Lmax : M;
        }
    }
    {
        const int wm = mb_wave_max_i32(Lmax);
        if ((tid & 63) == 0) atomicMax(&s_ref, wm);
    }
    __syncthreads();
    const int Rb = s_ref;
    bool fits = true;
    for (int x = tid; x < NE; x += 256) {
        const float L = sL[x];
        float c = 0.f;
        if (L > MB_DEADF) {
            if (L < (float)(Rb - 100)) fits = false;
            else c = sYv[x] * __builtin_amdgcn_exp2f((float)Rb - L);
        }
        sC[x] = c;
    }
    const int slow = __syncthreads_or(!fits);
    int lo, hi;
    mb_bounds(I, J, D, i, lo, hi);
#pragma unroll 1
    for (int q = 0; q < MB_NCH / 256; ++q) {
        const int x0 = tid + 256 * q, y = y0 + x0;
        if (y >= p.Ty) break;
        float gr = 0.f;
        const int m = y + 1;
        const float ev = (y < J) ? mb_value<VT>(mb_load_raw<VT>(p.e, ro + y)) : 0.f;
        if (y < J && m >= lo && m <= hi && p.log_alpha[ro + y] > MB_FINITE && ev > MB_FINITE && ev < -MB_FINITE) {
            const float e2 = ev * MB_LOG2E;
            float z = p.G[ro + y];
            if (i + 1 < I && m < p.Ty) z += p.Yw[ro + p.Ty + m];
            float flow;
            if (!slow) {
                const float *c = sC + x0;
                float acc = 0.f;
                int t = 0;
                for (; t + 8 <= D; t += 8)
                    acc += ((c[t] + c[t + 1]) + (c[t + 2] + c[t + 3])) + ((c[t + 4] + c[t + 5]) + (c[t + 6] + c[t + 7]));
                for (; t < D; ++t) acc += c[t];
                flow = (acc != 0.f) ? acc * __builtin_amdgcn_exp2f(e2 - (float)Rb) : 0.f;
            } else {
                flow = 0.f;
                for (int t = 0; t < D; ++t) {
                    const float L = sL[x0 + t];
                    if (L > MB_DEADF) flow += sYv[x0 + t] * __builtin_amdgcn_exp2f(e2 - L);
                }
            }
            gr = z - flow;
        }
        p.grad[ro + y] = gr;
    }
}
