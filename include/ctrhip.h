/*
 * ctrhip.h -- C ABI of libctrhip.so: hand-written gfx950 (MI355X) kernels for the
 * forward/backward of a CTR model zoo.
 *
 * The reference (WardellZc/DeepLearningRecommendationSystem) has no FFI layer:
 * its hot path is `model/<m>.py: nn.Module.forward` + autograd, called from
 * `trainer/trainer.py:23-40`.  These entry points are what a binding for that
 * path binds instead of ATen ops; each declaration names the reference lines
 * it replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the comment says "host";
 *  - tensors are fp32, row-major, with an explicit leading dimension in
 *    elements (ld*); indices are int64 as `nn.Embedding` takes them;
 *  - `stream` is a hipStream_t; every call only enqueues work on it, never
 *    allocates, never synchronises, keeps no state between calls and is
 *    re-entrant per stream (one caller-owned exception: the ticket word of
 *    ctr_bce_fwd, zero before and after every call);
 *  - return value: 0 = enqueued, <0 = CTR_E* (nothing enqueued).  Never
 *    throws, never exits.  ctr_strerror() names a code;
 *  - out-of-range indices never fault: the row is treated as row 0 and, when
 *    `err_flag` (device int32, may be NULL) is given, it is set to 1 so the
 *    host can raise the IndexError `nn.Embedding` would have raised.
 */
#ifndef CTRHIP_H
#define CTRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTR_OK 0
#define CTR_EINVAL (-1)   /* bad argument (null pointer, negative size, bad kind) */
#define CTR_ELIMIT (-2)   /* shape outside what the kernels are built for */
#define CTR_ELAUNCH (-3)  /* hipLaunchKernel reported an error */
#define CTR_EALIGN (-4)   /* pointer / leading dimension not aligned as required */

int ctr_version(void);                 /* ABI version, bumped on any signature change */
const char* ctr_strerror(int code);    /* host string, static storage */
const char* ctr_target_arch(void);     /* "gfx950" */

/* ------------------------------------------------------------------------
 * Embedding stage: fused row gather + weighted bag pooling + concat.
 * Replaces the nn.Embedding calls, the "multi-hot matmul" poolings and the
 * torch.cat that follows them:
 *   model/pnn.py:113-121, model/deepfm.py:45-54, model/deepcrossing.py:63-71,
 *   model/ffm.py:48-59, model/neuralcf.py:36-46, model/mf.py:24-25.
 * One launch writes, for every sample b and field f, `width` floats at
 * out[b*ldo + out_col ...].
 * ---------------------------------------------------------------------- */
enum {
  CTR_FIELD_ID_I64 = 0,  /* out = table[idx[b*idx_stride]]                        (K1/K3) */
  CTR_FIELD_ID_F32 = 1,  /* out = table[(int64)x[b*ldx+src_col]]  ("x[:,c].long()") (K1) */
  CTR_FIELD_BAG = 2,     /* out = sum_j x[b*ldx+src_col+j] * table[j], j<bag_size  (K2) */
  CTR_FIELD_DENSE = 3,   /* out = x[b*ldx+src_col .. +width)   (deepcrossing.py:65)      */
  CTR_FIELD_PROD_I64 = 4 /* out = table[idx[b]] * table2[idx2[b]] (neuralcf.py:36-39)    */
};
#define CTR_MAX_FIELDS 32

typedef struct ctr_field {
  int32_t kind;
  int32_t width;          /* floats written per sample (embedding dim E) */
  int32_t out_col;        /* first output column */
  int32_t src_col;        /* ID_F32 / BAG / DENSE: first column of x */
  int32_t bag_size;       /* BAG: K (table has K rows) */
  int32_t reserved;
  int64_t vocab;          /* rows of `table` (bounds check) */
  int64_t idx_stride;     /* ID_I64 / PROD: elements between consecutive samples */
  const int64_t* idx;     /* ID_I64 / PROD */
  const float* table;     /* (vocab, width) */
  float* grad;            /* backward: dense (vocab, width) accumulator, NULL = skip */
  const int64_t* idx2;    /* PROD only */
  const float* table2;    /* PROD only, (vocab2, width) */
  float* grad2;           /* PROD only */
  int64_t vocab2;         /* PROD only */
} ctr_field_t;

/* fields: host array of nfields (<= CTR_MAX_FIELDS) descriptors, copied by value */
int ctr_embed_fwd(const ctr_field_t* fields, int nfields, const float* x, int64_t ldx,
                  int64_t batch, float* out, int64_t ldo, int32_t* err_flag, void* stream);

/* backward of ctr_embed_fwd (autograd of the lines above; embedding_dense_backward
 * and the `x^T g` matmul backward, trainer/trainer.py:38): accumulates
 * (+=) into each field's dense `grad`; the caller zero-fills it first when it
 * wants a fresh gradient.  Id rows: fp32 atomics (order of accumulation not
 * fixed).  Bag tables (every sample hits the same few rows): reduced per
 * workgroup in LDS, then through `workspace` (device scratch, nullable; see
 * ctr_linear_bwd) or, without it, by atomics.  A sample whose id is out of
 * range (either id of a product field) adds to no row, on every path. */
int ctr_embed_bwd(const ctr_field_t* fields, int nfields, const float* x, int64_t ldx,
                  int64_t batch, const float* gout, int64_t ldo,
                  float* workspace, int64_t workspace_floats, void* stream);
/* ------------------------------------------------------------------------
 * Matrix factorisation, fused (model/mf.py:23-26):
 *   prob[b] = sigmoid(sum_e U[u[b],e] * V[i[b],e])
 * bwd: dlogit = gprob*prob*(1-prob); dU[u[b]] += dlogit*V[i[b]]; dV likewise.
 * ---------------------------------------------------------------------- */
int ctr_mf_fwd(const float* user_table, int64_t num_users, const float* item_table, int64_t num_items,
               int dim, const int64_t* user_idx, const int64_t* item_idx, int64_t batch,
               float* prob, int32_t* err_flag, void* stream);
int ctr_mf_bwd(const float* user_table, int64_t num_users, const float* item_table, int64_t num_items,
               int dim, const int64_t* user_idx, const int64_t* item_idx, int64_t batch,
               const float* prob, const float* gprob, float* guser, float* gitem, void* stream);

/* ------------------------------------------------------------------------
 * Dense layers (every nn.Linear of the zoo, e.g. model/neuralcf.py:48-51,57,
 * model/pnn.py:18-23,75-76, model/deepfm.py:57-60, model/din.py:14-29).
 *   Y[m, n] = act( sum_k X[m,k] * W[n,k] + bias[n] (+ R[m,n]) )
 * W is nn.Linear's (out_features, in_features) layout.  fp32 in, fp32 MFMA
 * accumulate (v_mfma_f32_32x32x2_f32), fp32 out.
 * ---------------------------------------------------------------------- */
enum { CTR_ACT_NONE = 0, CTR_ACT_RELU = 1, CTR_ACT_SIGMOID = 2 };

int ctr_linear_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias /*nullable*/,
                   const float* residual /*nullable*/, int64_t ldr,
                   float* y, int64_t ldy, int64_t m, int n, int k, int act, void* stream);

/* gz = gy * act'(y) (uses the saved OUTPUT y: relu mask y>0, sigmoid y(1-y));
 * gx[m,k] = sum_n gz[m,n] W[n,k]      (skipped when gx == NULL;  += when accumulate_gx)
 * gw[n,k] += sum_m gz[m,n] X[m,k]     (skipped when gw == NULL)
 * gb[n]  += sum_m gz[m,n]             (skipped when gb == NULL; needs gw: CTR_EINVAL, nothing enqueued)
 * Autograd of the nn.Linear + activation lines above (trainer/trainer.py:38).
 * gw/gb are sums over row chunks computed by different workgroups.  With a
 * `workspace` (device scratch, `workspace_floats` floats, may be NULL; 16M floats
 * give every layer of the zoo its full parallelism) each chunk stores its partial there and a second
 * pass adds them in a fixed order (reproducible); without it the chunks accumulate
 * with fp32 atomics.  Either way the result is ADDED to gw/gb: zero-fill for a
 * fresh gradient.  A workspace of any size is used for as many partials as it
 * holds (none: the atomics), but precision is not the same at every size: with
 * room for only a few partials of a wide layer (m >= 4096, n >= 96 or k >= 96)
 * each one adds m / partials rows in a single fp32 chain.  Measured at m = 4100
 * with room for 3: errors up to 0.98 of 2e-6 sqrt(m) + 1e-5 |gw|, against 0.4
 * with the 33 partials an ample workspace gets. */
int ctr_linear_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw,
                   const float* y, int64_t ldy, const float* gy, int64_t ldgy,
                   float* gx, int64_t ldgx, int accumulate_gx,
                   float* gw, int64_t ldgw, float* gb,
                   int64_t m, int n, int k, int act,
                   float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------
 * Feature interactions on the stacked embedding matrix emb (batch, >= nvec*dim)
 * written by ctr_embed_fwd: vector f of sample b is emb[b*lde + f*dim ...].
 * ---------------------------------------------------------------------- */

/* PNN inner products (model/pnn.py:59-66): out[b, idx(i,j)] = <v_i, v_j>, i<j in
 * lexicographic order, nvec*(nvec-1)/2 columns. */
int ctr_allpairs_fwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     float* out, int64_t ldo, void* stream);
/* gemb[b,i,:] (= or +=) sum_{j!=i} gp[b, idx(i,j)] * v_j */
int ctr_allpairs_bwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     const float* gp, int64_t ldgp, float* gemb, int64_t ldg, int accumulate, void* stream);

/* NFM bi-interaction pooling (model/nfm.py:56-61): out[b, e] = sum_{i<j} v_i[e] * v_j[e], pairs in
 * the reference's order; emb as for ctr_allpairs_fwd.  bwd: gemb[b,i,e] (= or +=) g[b,e] * sum_{j!=i} v_j[e]. */
int ctr_biinteract_fwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                       float* out, int64_t ldo, void* stream);
int ctr_biinteract_bwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                       const float* gout, int64_t ldgo, float* gemb, int64_t ldg, int accumulate, void* stream);

/* AFM pair products (model/afm.py:56-60): out[(b*np + idx(i,j))*ldo + e] = v_i[e] * v_j[e], i<j
 * lexicographic, np = nvec*(nvec-1)/2 rows per sample, nvec <= 16.
 * bwd: gpair = gp (+ attn[b*np + p] * gpool[b] when both are given: the attention-weighted sum
 * of afm.py:65); gemb[b,i,e] (= or +=) sum_{j!=i} gpair[b, idx(i,j), e] * v_j[e]. */
int ctr_pairprod_fwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     float* out, int64_t ldo, void* stream);
int ctr_pairprod_bwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     const float* gp, int64_t ldgp, const float* attn /*nullable*/,
                     const float* gpool /*nullable*/, int64_t ldgo,
                     float* gemb, int64_t ldg, int accumulate, void* stream);

/* N single-id fields, gather fused with the FM interaction (model/deepfm.py:45-46 applied to each of
 * F id columns, :63 first-order id terms, :71-77 second order; BASELINE configs[2] "26 fields x 1e6
 * vocab").  idx is the (batch, >= nfields) int64 id matrix (row stride ldidx); tables[f] is the
 * (vocabs[f], dim) table of field f, first[f] its (vocabs[f], 1) first-order weight (first or any
 * first[f] may be NULL); host arrays of device pointers.  dim in {8, 16, 32, 64}.
 *   emb[b, f*dim + e] = tables[f][idx[b,f], e]                       (bit-exact row copies)
 *   fm[b*ldfm] = (sum_f first[f][idx[b,f]] + bias[0]) + 0.5 * sum_e[(sum_f v_fe)^2 - sum_f v_fe^2]
 * A bad id reads row 0 and raises *err_flag (nullable). */
int ctr_fields_fm_fwd(const int64_t* idx, int64_t ldidx, int64_t batch, int nfields, int dim,
                      const float* const* tables, const int64_t* vocabs, const float* const* first /*nullable*/,
                      const float* bias /*nullable*/, float* emb, int64_t lde, float* fm, int64_t ldfm,
                      int32_t* err_flag, void* stream);
/* backward of the above for g = gfm[b*ldgfm] and the gradient gdeep (batch, nfields*dim) that the
 * consumers of emb returned (either may be NULL): dense scatter-add with fp32 atomics
 *   gtables[f][idx[b,f], e] += gdeep[b, f*dim+e] + g * (S_e - v_fe)   (v read back from emb, S_e = sum_f v_fe)
 *   gfirst[f][idx[b,f]] += g,   gbias[0] += sum_b g   (fixed-order partials through the workspace)
 * gtables[f] / gfirst / gfirst[f] / gbias may be NULL (frozen). */
int ctr_fields_fm_bwd(const int64_t* idx, int64_t ldidx, int64_t batch, int nfields, int dim, const int64_t* vocabs,
                      const float* emb, int64_t lde, const float* gdeep /*nullable*/, int64_t ldg,
                      const float* gfm /*nullable*/, int64_t ldgfm, float* const* gtables,
                      float* const* gfirst /*nullable*/, float* gbias /*nullable*/, float* workspace,
                      int64_t workspace_floats, void* stream);

/* the same two operations (same arguments, same results) for many vectors -- PNN over F id fields, 325 products at
 * F = 26 (model/pnn.py:59-66 applied to F fields).  The pinned shape F = 26, dim = 16 with 16-byte aligned, 4-float
 * padded prod / gp rows runs with all 26 vectors of a sample in the registers of a lane quad (forward 45 us,
 * backward 102 us at batch 65536 against 132 / 275 us of ctr_allpairs_*).  Other shapes: forward through a
 * wave-private LDS strip (dim in {8, 16, 32, 64}, F*dim floats x 256/dim samples <= 56 KB); backward returns
 * CTR_ELIMIT with nothing enqueued and the caller uses ctr_allpairs_bwd. */
int ctr_fields_pairs_fwd(const float* emb, int64_t lde, int64_t batch, int nfields, int dim,
                         float* prod, int64_t ldp, void* stream);
int ctr_fields_pairs_bwd(const float* emb, int64_t lde, int64_t batch, int nfields, int dim,
                         const float* gp, int64_t ldgp, float* gemb, int64_t ldg, int accumulate, void* stream);

/* DeepFM wide part + FM second order (model/deepfm.py:63,71-77):
 *   out[b*ldo] = user1[u] + item1[i] + (x[b, dense_col0..+ndense) . wide_w + wide_b)
 *               + 0.5 * sum_e[(sum_f v_fe)^2 - sum_f v_fe^2]
 * with u = (int64)x[b,user_col], i = (int64)x[b,item_col]; user1/item1 are the
 * (vocab,1) tables `self.user` / `self.item`, wide_w the (1,ndense) weight. */
int ctr_fm_wide_fwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                    const float* x, int64_t ldx, int user_col, int item_col, int dense_col0, int ndense,
                    const float* user1, int64_t num_users, const float* item1, int64_t num_items,
                    const float* wide_w, const float* wide_b, float* out, int64_t ldo,
                    int32_t* err_flag, void* stream);
/* g = gout[b*ldgo]: guser1[u] += g, gitem1[i] += g, gwide_w += sum_b g x, gwide_b += sum_b g,
 * gemb[b,f,e] (= or +=) g * (sum_f' v_f'e - v_fe).  Any grad pointer may be NULL. */
int ctr_fm_wide_bwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                    const float* x, int64_t ldx, int user_col, int item_col, int dense_col0, int ndense,
                    const float* user1, int64_t num_users, const float* item1, int64_t num_items,
                    const float* wide_w, const float* wide_b, const float* gout, int64_t ldgo,
                    float* guser1, float* gitem1, float* gwide_w, float* gwide_b,
                    float* gemb, int64_t ldg, int accumulate,
                    float* workspace, int64_t workspace_floats, void* stream);

/* FFM head (model/ffm.py:62-86): cross = sum_p <v_a(p), v_b(p)> over the host pair
 * list `pairs` (2*npairs ints, npairs <= 64), summed left to right;
 *   prob[b*ldo] = sigmoid(user1[u] + item1[i] + sum_c (x[b,c] + cross) * lin_w[c] + lin_b)
 * -- the reference adds the cross scalar to every dense input before its linear
 * layer (ffm.py:84-86) and so does this. */
int ctr_ffm_head_fwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     const int32_t* pairs, int npairs,
                     const float* x, int64_t ldx, int user_col, int item_col, int dense_col0, int ndense,
                     const float* user1, int64_t num_users, const float* item1, int64_t num_items,
                     const float* lin_w, const float* lin_b, float* prob, int64_t ldo,
                     int32_t* err_flag, void* stream);
int ctr_ffm_head_bwd(const float* emb, int64_t lde, int64_t batch, int nvec, int dim,
                     const int32_t* pairs, int npairs,
                     const float* x, int64_t ldx, int user_col, int item_col, int dense_col0, int ndense,
                     const float* user1, int64_t num_users, const float* item1, int64_t num_items,
                     const float* lin_w, const float* lin_b,
                     const float* prob, int64_t ldp, const float* gprob, int64_t ldgp,
                     float* guser1, float* gitem1, float* glin_w, float* glin_b,
                     float* gemb, int64_t ldg,
                     float* workspace, int64_t workspace_floats, void* stream);

/* out (= or +=) gy * act'(y): the residual branch of model/deepcrossing.py:26 */
int ctr_act_bwd(const float* y, int64_t ldy, const float* gy, int64_t ldgy, float* out, int64_t ldo,
                int64_t m, int n, int act, int accumulate, void* stream);

/* ------------------------------------------------------------------------
 * Cross layer of Deep & Cross (model/deepcross.py:7-18):
 *   x_{l+1} = x0 * (W_l x_l) + b_l + x_l,  W_l a bias-free (d, d) nn.Linear.
 * u = x_l W_l^T is a ctr_linear_fwd call; these are the combine around it.
 *   fwd: y[m,d] = x0 * u + bias + xl
 *   bwd: gu = gy * x0 (operand of the layer's dX / dW, i.e. ctr_linear_bwd with gy := gu),
 *        gx0 += gy * u, gbias += column sums of gy (through `workspace`, fixed order).
 *        The gradient w.r.t. x_l is gy + gu W_l: accumulate the dX of ctr_linear_bwd
 *        (accumulate_gx) into the gy buffer.   d <= 1024.
 * ---------------------------------------------------------------------- */
int ctr_cross_fwd(const float* x0, int64_t ldx0, const float* u, int64_t ldu, const float* xl, int64_t ldxl,
                  const float* bias, float* y, int64_t ldy, int64_t m, int d, void* stream);
int ctr_cross_bwd(const float* x0, int64_t ldx0, const float* u, int64_t ldu, const float* gy, int64_t ldgy,
                  float* gu, int64_t ldgu, float* gx0, int64_t ldgx0, float* gbias, int64_t m, int d,
                  float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------
 * DIN / DIEN attention over the behaviour sequence (model/din.py:33-53,
 * model/dien.py:23-39).  hist is (batch, len) int64 row-major, target (batch,).
 * ---------------------------------------------------------------------- */

/* K3 sequence gather fused with the attention operand (din.py:35-42):
 *   CTR_DIN_TRIPLE: c[(b*len+l)*ldc + 0:E] = h, [E:2E] = h - t, [2E:3E] = t   (the reference's cat)
 *   CTR_DIN_PAIR:   c[(b*len+l)*ldc + 0:E] = h, [E:2E] = t.  Since W.[h, h-t, t] =
 *                   (Wa+Wb).h + (Wc-Wb).t, a caller that folds the first attention layer's weight
 *                   columns this way gets the same layer output from a 2E-wide operand (2/3 of
 *                   the bytes and flops of the largest GEMM of the step).
 *   h = table[hist[b,l]], t = table[target[b]];  tvec[b*ldt + 0:E] = t  (tvec may be NULL). */
enum { CTR_DIN_TRIPLE = 0, CTR_DIN_PAIR = 1, CTR_DIN_H = 2 /* forward only: c[(b*len+l)*ldc + 0:E] = h, the E-wide operand */ };
int ctr_din_concat_fwd(const float* table, int64_t vocab, int dim, const int64_t* hist, const int64_t* target,
                       int64_t batch, int len, float* c, int64_t ldc, float* tvec, int64_t ldt, int layout,
                       int32_t* err_flag, void* stream);
/* attn[b,:] = softmax_len(score[b,:]) with no padding mask (din.py:44); h_l is read
 * from hsrc[(b*len+l)*ldh ...].  summed != 0: out[b*ldo ...] = sum_l attn_l h_l
 * (din.py:47); summed == 0: out[(b*len+l)*ldo ...] = attn_l h_l (dien.py:37). */
int ctr_din_pool_fwd(const float* score, const float* hsrc, int64_t ldh, int64_t batch, int len, int dim,
                     float* attn, float* out, int64_t ldo, int summed, void* stream);
/* gradient of the scores through pooling + softmax; gout as `out` above */
int ctr_din_pool_bwd(const float* attn, const float* hsrc, int64_t ldh, int64_t batch, int len, int dim,
                     const float* gout, int64_t ldgo, int summed, float* gscore, void* stream);
/* every gradient path into the dense item-table gradient (+=, fp32 atomics):
 *   CTR_DIN_TRIPLE: row hist[b,l] += gc[.,0:E] + gc[.,E:2E] + attn[b,l] * gout_l
 *                   row target[b] += sum_l (gc[.,2E:3E] - gc[.,E:2E]) + gt_extra[b]
 *   CTR_DIN_PAIR:   row hist[b,l] += gc[.,0:E] + attn[b,l] * gout_l
 *                   row target[b] += sum_l gc[.,E:2E] + gt_extra[b]          (gt_extra may be NULL) */
int ctr_din_concat_bwd(const int64_t* hist, const int64_t* target, int64_t vocab, int64_t batch, int len, int dim,
                       const float* gc, int64_t ldc, const float* attn, const float* gout, int64_t ldgo,
                       int summed, const float* gt_extra, int64_t ldgt, int layout, float* gtable, void* stream);

/* ------------------------------------------------------------------------
 * DIEN interest evolution: nn.GRU(E, E, batch_first=True), one layer, h0 = 0
 * (model/dien.py:47,61), dim <= 64.  gi = X W_ih^T + b_ih for all steps is a
 * ctr_linear_fwd call; these run the recurrence.
 *   hbuf: (batch, len+1, dim), hbuf[b,0,:] = 0, hbuf[b,t+1,:] = h_t; `last`
 *   (nullable) receives hidden[-1] = h_{len-1} at last[b*ldl ...].
 * Backward writes dgi (batch*len, 3*dim) and dgh (batch, len+1, 3*dim; row 0 zero,
 * row t+1 = gradient of W_hh h_{t-1} + b_hh), from which
 *   dW_ih = dgi^T X, db_ih = sum dgi, dX = dgi W_ih,
 *   dW_hh = dgh[1:]^T hbuf[:-1], db_hh = sum dgh       are ctr_linear_bwd calls.
 * ---------------------------------------------------------------------- */
int ctr_gru_fwd(const float* gi, int64_t ldgi, const float* w_hh, const float* b_hh, int64_t batch, int len,
                int dim, float* hbuf, float* last, int64_t ldl, void* stream);
int ctr_gru_bwd(const float* gi, int64_t ldgi, const float* w_hh, const float* b_hh, const float* hbuf,
                int64_t batch, int len, int dim, const float* glast, int64_t ldgl, float* dgi, float* dgh,
                void* stream);
/* The same GRU with the input projection inside: x (batch*len, dim) rows instead of gi, W_ih (3*dim, dim), b_ih.
 * Forward writes hbuf / last as ctr_gru_fwd.  Backward recomputes the projection and leaves, instead of dgi / dgh,
 *   gx (batch*len, dim) = dgi W_ih,   gw_ih += dgi^T X,  gb_ih += sum dgi,  gw_hh += dgh^T H_prev,  gb_hh += sum dgh
 * (weight sums per workgroup in registers, fixed-order partials through the workspace: >= 256 * 1632 floats).
 * dim == 16 only (CTR_ELIMIT otherwise with nothing enqueued -- use ctr_linear_fwd + ctr_gru_fwd / ctr_gru_bwd +
 * ctr_linear_bwd as above).  With 16-byte aligned x / hbuf / gx rows (ldx, ldgx multiples of 4) the recurrence runs on
 * the matrix cores, sixteen samples per wave, for any batch; otherwise on DPP rows of four samples, batch % 4 == 0. */
int ctr_gru_fused_fwd(const float* x, int64_t ldx, const float* w_ih, const float* b_ih, const float* w_hh,
                      const float* b_hh, int64_t batch, int len, int dim, float* hbuf, float* last /*nullable*/,
                      int64_t ldl, void* stream);
int ctr_gru_fused_bwd(const float* x, int64_t ldx, const float* w_ih, const float* b_ih, const float* w_hh,
                      const float* b_hh, const float* hbuf, int64_t batch, int len, int dim, const float* glast,
                      int64_t ldgl, float* gx, int64_t ldgx, float* gw_ih, float* gb_ih, float* gw_hh, float* gb_hh,
                      float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------
 * A whole stack of narrow nn.Linear(+activation) layers in one launch (forward) and
 * one launch (backward): e.g. NeuralCF's tower, model/neuralcf.py:48-51.  A wave
 * carries 32 rows through every layer with the activations in LDS and all weights
 * of the stack resident in LDS.  Limits: <= 8 layers, every k a multiple of 8 and
 * <= 128, every n <= 128, k[i] == n[i-1], weights 16-byte aligned, intermediate
 * outputs 16-byte aligned with ldy % 4 == 0.  Anything else returns CTR_ELIMIT /
 * CTR_EALIGN without enqueueing; use ctr_linear_* layer by layer then.
 * Which code: CTR_ELIMIT for a shape the kernels are not built for (more than 8
 * layers, n or k above 128, k not a multiple of 8, a stack that does not fit LDS,
 * more than 16 dW tiles of 32 x 32 in the backward, fewer workspace floats than
 * the backward needs, head: p above 64, p not a multiple of 8, p + n_last above 192);
 * CTR_EALIGN for x, an intermediate y or the head's x off a 16-byte boundary or
 * with a leading dimension that is no multiple of 4.  A stack that no path could
 * run is CTR_EINVAL, also without enqueueing: k < 8, k[i] != n[i-1], a null w or y,
 * ldy < n, w off a 16-byte boundary, an unknown activation, and in the backward a
 * layer without gw or gb (gb is required even where the forward's b was NULL).
 * m == 0 is CTR_OK and enqueues nothing.
 * ---------------------------------------------------------------------- */
typedef struct ctr_mlp_layer {
  const float* w;   /* (n, k) row-major */
  const float* b;   /* (n) or NULL */
  float* y;         /* forward: output (m, ldy), kept for backward; backward: read */
  int64_t ldy;
  float* gw;        /* backward: (n, k), accumulated into (+=) */
  float* gb;        /* backward: (n),   accumulated into (+=) */
  int32_t n, k, act;
  int32_t reserved;
} ctr_mlp_layer_t;

/* y_0 = act_0(x W_0^T + b_0), y_i = act_i(y_{i-1} W_i^T + b_i); layers: host array */
int ctr_mlp_fwd(const float* x, int64_t ldx, int64_t m, const ctr_mlp_layer_t* layers, int nlayers,
                void* stream);
/* The same stack with a single-unit head formed in its epilogue, while the last activations are still
 * on chip:  out[row*ldout] = act( x_extra[row, 0:p] . w[0:p] + y_last[row, :] . w[p:] + c[0] ).
 * NeuralCF's folded linear2 (see ctr_fold_head_fwd): x_extra = the GMF product, w = wfold, c = cfold.
 * The stack's own outputs are written as by ctr_mlp_fwd.  Limits: p <= 64 and a multiple of 8, x_extra
 * rows 16-byte aligned (else CTR_ELIMIT / CTR_EALIGN, nothing enqueued). */
typedef struct ctr_mlp_head {
  const float* x;   /* (m, ldx): p extra input columns, or NULL when p == 0 */
  int64_t ldx;
  const float* w;   /* p + n_last weights */
  const float* c;   /* one bias (device) */
  float* out;       /* (m) at stride ldout */
  int64_t ldout;
  int32_t p, act;
} ctr_mlp_head_t;
int ctr_mlp_head_fwd(const float* x, int64_t ldx, int64_t m, const ctr_mlp_layer_t* layers, int nlayers,
                     const ctr_mlp_head_t* head, void* stream);
/* The embedding stage and the stack behind it in one launch: the effect of
 *   ctr_embed_fwd(fields, nfields, NULL, 0, batch, out, ldo, err_flag)  followed by
 *   ctr_mlp_head_fwd(out, ldo, batch, layers, nlayers, head)            with head->x inside `out`,
 * for the pattern the library has a kernel for -- NeuralCF at BASELINE configs[1] (model/neuralcf.py:37-56:
 * fields = [ID_I64 64 -> column 0, ID_I64 64 -> column 64, PROD_I64 64 -> column 128] of one matrix, the pinned
 * 128-64-32-16-8 ReLU tower on columns 0..127, head->x = out + 128, p = 64).  The kernel reads the ids and table rows
 * itself.  The product columns (head->x) are always written; the tower's input columns 0..127 only with
 * write_x != 0 -- with write_x == 0 they stay untouched and the backward must be ctr_embed_mlp_head_bwd, which
 * gathers them again.  Any other shape: CTR_ELIMIT, nothing enqueued -- issue the two calls. */
/* optional: ctr_fold_head_fwd's map done by the same launch (NULL: head->w / head->c are read as they are).  The
 * kernel forms wfold = [u_full[:p] | W^T u_full[p:]] and cfold = b . u_full[p:] + b2 itself and also writes them to
 * `wfold` / `cfold`, which must be the buffers head->w / head->c point at (the backward reads them there). */
typedef struct ctr_head_fold {
  const float* u_full;  /* (p + n) */
  const float* w;       /* (n, k) at row stride ldw */
  int64_t ldw;
  const float* b;       /* (n) or NULL */
  const float* b2;      /* (1) or NULL */
  float* wfold;         /* (p + k), == head->w */
  float* cfold;         /* (1),     == head->c */
  int32_t p, n, k, reserved;
} ctr_head_fold_t;
int ctr_embed_mlp_head_fwd(const ctr_field_t* fields, int nfields, int64_t batch, float* out, int64_t ldo,
                           int32_t* err_flag /*nullable*/, int write_x, const ctr_mlp_layer_t* layers, int nlayers,
                           const ctr_mlp_head_t* head, const ctr_head_fold_t* fold /*nullable*/, void* stream);
/* Backward of ctr_mlp_head_fwd in ONE launch with the stack's backward: per row gz = gprob * act'(prob);
 * the stack's gY is gz * w[p:] (never stored), gx_extra[row, 0:p] = gz * w[0:p] is written, and
 * gw[0:p+n_last] += sum_rows gz * [x_extra | y_last],  gc[0] += sum_rows gz.  Layers' gw / gb and gx as in
 * ctr_mlp_bwd.  Available for the pinned NeuralCF tower (128-64-32-16-8, relu) with p == 64 only; any other
 * stack returns CTR_ELIMIT without enqueueing (then: ctr_linear_bwd on the head + ctr_mlp_bwd).
 * workspace: (workgroups <= 256) * (sum_i (n_i*k_i + n_i) + p + n_last + 1) floats. */
typedef struct ctr_mlp_head_grad {
  const float* prob;  int64_t ldprob;   /* head output (m), as written by ctr_mlp_head_fwd */
  const float* gprob; int64_t ldgprob;  /* its gradient (m) */
  const float* x;     int64_t ldx;      /* the p extra input columns */
  const float* w;                       /* p + n_last head weights */
  float* gx;          int64_t ldgx;     /* gradient of the extra columns, written (=) */
  float* gw;                            /* p + n_last, accumulated */
  float* gc;                            /* 1, accumulated */
  int32_t p, act;
} ctr_mlp_head_grad_t;
int ctr_mlp_head_bwd(const float* x, int64_t ldx, int64_t m, const ctr_mlp_layer_t* layers, int nlayers,
                     const ctr_mlp_head_grad_t* head, float* gx, int64_t ldgx, float* workspace,
                     int64_t workspace_floats, void* stream);
/* ctr_mlp_head_bwd for a forward done by ctr_embed_mlp_head_fwd(..., write_x = 0, ...): the stack's input
 * [table[idx] | table[idx]] of the first two fields is gathered again by the samples' ids (out-of-range ids read
 * row 0, as in the forward) instead of being read from memory; hg->x is the product columns the forward wrote.
 * Same outputs and workspace contract as ctr_mlp_head_bwd.  CTR_ELIMIT: not the pattern, nothing enqueued. */
/* optional (NULL: hg->gw / hg->gc only): ctr_fold_head_bwd done by the reduction launch of the same call, from the
 * totals hg->gw (p + k) / hg->gc hold afterwards -- same arguments and (+=) semantics as ctr_fold_head_bwd. */
typedef struct ctr_head_fold_grad {
  const float* u_full;  /* (p + n) */
  const float* w;       /* (n, k) at row stride ldw */
  int64_t ldw;
  const float* b;       /* (n) or NULL */
  float* gu_full;       /* (p + n) or NULL */
  float* gw;            /* (n, k) at row stride ldgw, or NULL */
  int64_t ldgw;
  float* gb;            /* (n) or NULL */
  float* gb2;           /* (1) or NULL */
  int32_t p, n, k, reserved;
} ctr_head_fold_grad_t;
/* zero_buf (nullable; 16-byte aligned, zero_floats a multiple of 4): cleared by the first launch of the call, before
 * anything accumulates -- the buffer the (+=) outputs of this step live in (torch's optimizer.zero_grad / the fill
 * launch in front of the backward).  On CTR_ELIMIT nothing was enqueued and nothing was cleared. */
int ctr_embed_mlp_head_bwd(const ctr_field_t* fields, int nfields, int64_t batch, const ctr_mlp_layer_t* layers,
                           int nlayers, const ctr_mlp_head_grad_t* hg, const ctr_head_fold_grad_t* fold /*nullable*/,
                           float* gx, int64_t ldgx, float* workspace, int64_t workspace_floats,
                           float* zero_buf /*nullable*/, int64_t zero_floats, void* stream);
/* ------------------------------------------------------------------------
 * A first Linear on a concatenation of two gathered rows, with the layer applied to the TABLE ROWS (any width; the
 * projected tables A = T_a W_a^T, B = T_b W_b^T + bias are two ctr_linear_fwd calls over the tables):
 *   out[b, :] = act(A[idx_a[b], :] + B[idx_b[b], :])                (model/neuralcf.py:43-49 for any tower)
 * An id outside its table reads row 0 and raises *err_flag.  Backward: ctr_act_mask_bwd turns the gradient of `out`
 * into the gradient of the pre-activation in place (g *= act'(out)); ctr_embed_bwd with two id fields on the same
 * gradient columns forms the row sums S_a, S_b; ctr_linear_bwd over the table rows turns them into the tables' and the
 * layer's gradients (dT = S W, dW = S^T T). */
int ctr_rows_sum_act_fwd(const float* table_a, const int64_t* idx_a, int64_t stride_a, int64_t vocab_a,
                         const float* table_b, const int64_t* idx_b, int64_t stride_b, int64_t vocab_b,
                         int64_t batch, int width, int act, float* out, int64_t ldo, int32_t* err_flag /*nullable*/,
                         void* stream);
int ctr_act_mask_bwd(float* g, int64_t ldg, const float* y, int64_t ldy, int64_t m, int n, int act, void* stream);

/* ------------------------------------------------------------------------
 * NeuralCF (model/neuralcf.py:33-59) when the vocabularies are much smaller than the batch: the first tower layer and
 * its whole backward are moved from the samples to the table rows.  Linear(cat(MLP_U[u], MLP_I[i])) ==
 * (MLP_U W0a^T)[u] + (MLP_I W0b^T + b0)[i]: two products over num_users + num_items rows instead of one over the
 * batch; backward: segment sums S_U / S_I of ONE 64-float row per sample, then dMLP = S W0half, dW0half = S^T MLP,
 * db0 = colsum S_U; the GMF tables' gradients and the head's GMF weights from T_U[u] = sum_b gz_b GMF_I[i_b]
 * likewise (csrc/ncf_proj.hip has the derivation).  Same function, same gradients as the per-sample path
 * (ctr_embed_mlp_head_fwd / _bwd) up to fp32 summation order.
 *
 * Pattern (anything else: CTR_ELIMIT, nothing enqueued -- use the per-sample entry points): mlp_dim == mf_dim == 64,
 * layers = {128->64, 64->32, 32->16, 16->8} all ReLU with biases, proj (`linear`) 8 -> 64, head (`linear2`) on
 * [gmf | linear(h)] (128 weights), num_users + num_items <= CTR_NCF_PROJ_MAX_ROWS, 16-byte aligned tables.
 * layers[0].y is not used (the first layer's output never exists per sample); layers[1..3].y are the saved
 * activations (m + 1, 32), (m + 1, 16), (m + 1, 8) the forward writes and the backward reads.  EVERY per-sample
 * buffer has one spare row behind the batch (prob: m + 1 elements; ranks: 2 (m + 1) int32): lanes without a sample
 * store / read there, so that no store of the per-sample kernels is conditional.
 * Caller-owned buffers the forward fills for the backward: ptab (num_users + num_items, 64), wfold (76 floats), and
 * with training != 0: ranks (a sample's rank among the samples of its chunk of the batch that carry its user id, and
 * the same for its item id) and plan ((num_users + num_items) * CTR_NCF_PROJ_COUNT_STRIDE int32: the bucket plan the
 * forward builds from the ids -- per table row the sample counts of up to 64 chunks of the batch as exclusive
 * prefixes with the row's bucket offset added, the row's total, the bucket offsets, per chunk its samples in every
 * block of 256 rows -- and the backward reads; csrc/ncf_proj.hip has the layout).  The forward writes every entry of
 * the plan that is read later and never touches its first four words: nothing has to be cleared between steps (a
 * caller that zero-fills the buffer once finds word 0 still zero).
 * The plan belongs to ONE forward until its backward has run: two forwards in flight need a buffer each.
 * Parameters must not change between the forward and the backward (the backward re-reads tables and ptab).
 * The backward's workspace (ctr_ncf_proj_workspace_floats): gz0 rows in sample order (batch + 1, 64) | slot records
 * (2 batch + 1, 4) = {gz, partner id, row, sample}, the user rows' buckets first | segment sums (rows, 128) | the
 * per-sample kernel's slabs.
 * The backward with the loss inside (ctr_ncf_proj_grad_t.target set): the gradient of prob is not passed in, it is
 * the binary cross entropy's for an upstream gradient of exactly 1 -- (p - y) / max(p (1 - p), 1e-12) / batch, the
 * expression and the bits of ctr_bce_fwd's gprob_unit -- formed by the per-sample kernel from prob and target; gprob
 * is then not read and may be null.  With `loss` set as well the call STORES the mean loss there (ctr_bce_fwd's
 * value up to fp32 summation order, the same bits from run to run): the per-sample kernel sums the terms, the last
 * launch adds the workgroups' sums in a fixed order, so the word is valid once launch 4 of `phases` has run.  No
 * launch, ticket or buffer is added.  Refused with CTR_EINVAL before anything is enqueued: `loss` without `target`,
 * ldtarget < 1, neither target nor gprob, and `loss` with an empty batch (there is no mean over no samples). */
#define CTR_NCF_PROJ_MAX_ROWS 16384
#define CTR_NCF_PROJ_COUNT_STRIDE 72   /* int32 of plan per table row: 64 chunk counts, total, offset, and room for the head and the block totals */
typedef struct ctr_ncf_proj {
  const int64_t* user_idx; int64_t user_stride;   /* ids of the batch, element strides */
  const int64_t* item_idx; int64_t item_stride;
  int64_t batch, num_users, num_items;
  const float* mlp_user; const float* mlp_item;   /* (num, mlp_dim) MLP_Embedding_User / _Item */
  const float* gmf_user; const float* gmf_item;   /* (num, mf_dim)  GMF_Embedding_User / _Item */
  int32_t mlp_dim, mf_dim;
  ctr_mlp_layer_t layers[4];                      /* dnn_network (gw / gb unused here) */
  const float* proj_w; int64_t ld_proj_w; const float* proj_b; int32_t proj_n, proj_k;   /* `linear` (proj_n, proj_k) */
  const float* head_w; const float* head_b; int32_t head_act;                            /* `linear2` (1, 2 mf_dim) */
  float* prob; int64_t ldprob;                    /* (batch) output */
  int32_t* err_flag;                              /* nullable */
  float* ptab; float* wfold; int32_t* plan; int32_t* ranks;
  int32_t training;
  int32_t phases;                                 /* 0: the whole call; else a mask of its launches (forward: 1 projected tables
                                                     + head fold, 2 per-sample kernel) -- for per-kernel timing */
} ctr_ncf_proj_t;
typedef struct ctr_ncf_proj_grad {
  const float* gprob; int64_t ldgprob;
  ctr_mlp_layer_t layers[4];                      /* gw / gb of dnn_network (+=); other members unused */
  float* g_mlp_user; float* g_mlp_item; float* g_gmf_user; float* g_gmf_item;   /* dense table gradients (+=) */
  float* g_proj_w; int64_t ld_g_proj_w; float* g_proj_b; float* g_head_w; float* g_head_b;   /* (+=) */
  float* workspace; int64_t workspace_floats;     /* >= ctr_ncf_proj_workspace_floats(batch, users, items) */
  float* zero_buf; int64_t zero_floats;           /* nullable: cleared by the call's first launch (see ctr_embed_mlp_head_bwd) */
  int32_t phases; int32_t reserved;               /* 0: the whole call; else a mask (1 per-sample kernel, 2 segment sums, 4 table-row
                                                     products + slab reduction + head fold), issued in that order */
  const float* target; int64_t ldtarget;          /* nullable: (batch) BCE targets, element stride; set: gprob is not read */
  float* loss;                                    /* nullable, only with target: the mean BCE loss is stored here */
} ctr_ncf_proj_grad_t;
int ctr_ncf_proj_workspace_floats(int64_t batch, int64_t num_users, int64_t num_items, int64_t* floats /*host, out*/);
int ctr_ncf_proj_fwd(const ctr_ncf_proj_t* d, void* stream);
int ctr_ncf_proj_bwd(const ctr_ncf_proj_t* d, const ctr_ncf_proj_grad_t* g, void* stream);

/* NeuralCF over the user x item grid (csrc/ncf_grid.hip): the scores of `rows` users against EVERY item in one launch,
 * with no id tensor:
 *   out[r * ldo + i] = act([gmf_user[u_r] * gmf_item[i] | tower(relu(p_user[u_r] + p_item[i]))] . wfold + cfold[0])
 *   u_r = users[r] (users set: any order, repeats allowed) or user0 + r (users NULL; user0 + rows <= num_users)
 * p_user (num_users, width) / p_item (num_items, width) are the first tower layer applied to the table rows
 * (MLP_U W0a^T and MLP_I W0b^T + b0: two ctr_linear_fwd), `layers` the nlayers REMAINING tower layers (w, b, n, k, act
 * read; rows of w contiguous), wfold (mf_dim + fold_k) / cfold (1) what ctr_fold_head_fwd writes.
 * Pattern, the one of ctr_ncf_proj_fwd (anything else: CTR_ELIMIT, nothing enqueued): mf_dim == width == 64, layers
 * 64->32, 32->16, 16->8 all ReLU with biases, fold_k == 8; num_users, num_items < 2^31.  There is NO cap on the table
 * rows (CTR_NCF_PROJ_MAX_ROWS belongs to the training plan).  Tables and weights 16-byte aligned (CTR_EALIGN).
 * out is (rows, num_items) float32 with row stride ldo >= num_items; columns past num_items are not touched.
 * A null table, layer array, wfold or cfold, ldo < num_items, a negative count or a row range outside the user table
 * is CTR_EINVAL before anything is enqueued; rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.  The
 * caller validates `users`: an id outside [0, num_users) is clamped into the table, not reported.  No atomics; a
 * pair's score is a function of its two table rows and the weights alone, bitwise, whatever the rows or their order. */
int ctr_ncf_grid_scores(const float* p_user, const float* p_item, const float* gmf_user, const float* gmf_item,
                        int64_t num_users, int64_t num_items, int mf_dim, int width,
                        const ctr_mlp_layer_t* layers, int nlayers, const float* wfold, const float* cfold, int fold_k,
                        const int64_t* users /*nullable*/, int64_t user0, int64_t rows, int act,
                        float* out, int64_t ldo, void* stream);

/* DIN over the history x item grid (csrc/din_grid.hip): the attention-pooled history of `rows` history rows against
 * EVERY item in one launch, with no id tensor and nothing written per history position:
 *   s[l]   = w3 . relu(w2 relu(AH[r, l] + at[i]) + b2)            (n1 = 128 -> n2 = 64 -> 1; the score bias drops out)
 *   out[(r * num_items + i) * ldo + 0:embed] = sum_l softmax_l(s)[l] table[hist[r * len + l]]      (no padding mask)
 *   AH[r, l] = ah[hist[r * len + l]] (ah_by_position == 0: ah is (num_items, n1)) or ah[r * len + l] (!= 0: ah is
 *   (rows * len, n1), the projection of the gathered history rows)
 * at (num_items, n1) = (Wc - Wb) table^T + b1 and ah = (Wa + Wb) h^T are two ctr_linear_fwd of the caller's; all
 * matrices are dense row-major.  Admitted: embed == 64, n1 == 128, n2 == 64, len >= 1, num_items < 2^31, ldo >= embed
 * and a multiple of 4, table / at / ah / w2 / out 16-byte aligned; anything else, or a null pointer, is CTR_EINVAL
 * before anything is enqueued.  rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.  Columns past `embed`
 * of a row of out are not touched.  A history id outside [0, num_items) is read as row 0 and sets *err_flag (nullable)
 * to 1, the convention of ctr_din_concat_fwd.  No atomics; a pair's row is a function of its history row, its item
 * and the weights alone, bitwise, whatever the rows, their order or the items' positions. */
int ctr_din_grid_pool(const float* table, int64_t num_items, int embed, const float* at, const float* ah,
                      int ah_by_position, const float* w2, const float* b2, const float* w3, int n1, int n2,
                      const int64_t* hist, int64_t rows, int len, float* out, int64_t ldo, int32_t* err_flag,
                      void* stream);

/* DIEN over the history x item grid (csrc/dien_grid.hip): the last GRU state of `rows` history rows against EVERY item
 * in one launch, with no id tensor and nothing written per history position:
 *   s[l]  = w3 . relu(w2 relu(AH[r, l] + at[i]) + b2)             (n1 = 64 -> n2 = 32 -> 1; the score bias drops out)
 *   a     = softmax_l(s);   gi_l = a[l] GX[r, l] + b_ih;   gh = w_hh h + b_hh            (gate order r, z, n; h_0 = 0)
 *   r = sig(gi_r + gh_r);  z = sig(gi_z + gh_z);  n = tanh(gi_n + r gh_n);  h <- (1 - z) n + z h
 *   out[(r * num_items + i) * ldo + 0:embed] = h after the row's last position           (no padding mask)
 *   [AH | GX][r, l] = hp[hist[r * len + l]] (hp_by_position == 0: hp is (num_items, n1 + 3 embed)) or hp[r * len + l]
 *   (!= 0: hp is (rows * len, n1 + 3 embed), the projection of the gathered history rows)
 * at (num_items, n1) = (Wc - Wb) table^T + b1 and hp = [Wa + Wb ; W_ih] h^T (no bias) are two ctr_linear_fwd of the
 * caller's; all matrices are dense row-major.  The scores of the first CTR_DIEN_GRID_KEEP positions of a row wait in
 * LDS for the recurrence, later ones are computed a second time (same instructions, same bits): any len >= 1 is taken.
 * Admitted: embed == 16, n1 == 64, n2 == 32, num_items < 2^31, anything else is CTR_ELIMIT; a null pointer, a negative
 * count, len < 1 or ldo < embed is CTR_EINVAL; at / hp / w2 / out not 16-byte aligned or ldo not a multiple of 4 is
 * CTR_EALIGN -- all before anything is enqueued.  rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.
 * Columns past `embed` of a row of out are not touched.  A history id outside [0, num_items) is read as row 0 and sets
 * *err_flag (nullable) to 1, the convention of ctr_din_concat_fwd.  No atomics; a pair's row is a function of its
 * history row, its item and the weights alone, bitwise, whatever the rows, their order or the items' positions. */
#define CTR_DIEN_GRID_KEEP 128
int ctr_dien_grid_hidden(const float* at, const float* hp, int hp_by_position, int64_t num_items, int embed,
                         const float* w2, const float* b2, const float* w3, int n1, int n2, const float* b_ih,
                         const float* w_hh, const float* b_hh, const int64_t* hist, int64_t rows, int len, float* out,
                         int64_t ldo, int32_t* err_flag, void* stream);

/* DeepFM over the user x item grid (csrc/deepfm_grid.hip): the scores of `rows` users against EVERY item in one launch,
 * with no feature matrix.  Every column of the (B, 45) feature row belongs to the user or to the item and the first
 * deep layer has no activation, so the model splits into table rows the caller makes with ctr_embed_fwd and
 * ctr_linear_fwd:
 *   h2 = relu(w2 relu(zu[u_r] + zi[i]) + b2)                                     (n1 = 256 -> n2 = 128)
 *   out[r * ldo + i] = sigmoid(out_w[0] (a[u_r] + b[i] + <su[u_r], si[i]>) + out_w[1] relu(w3 . h2 + b3[0]) + out_b[0])
 *   u_r = users[r] (users set: any order, repeats allowed) or user0 + r (users NULL; user0 + rows <= num_users)
 * zu (num_users, n1) / zi (num_items, n1): the deep layers in front of w2 applied to a side's columns of the embedding
 * row (the biases on the item side); su (num_users, embed) / si (num_items, embed): the sums of a side's field vectors;
 * a / b: the side's first-order, wide and 0.5 (|sum|^2 - sum |f|^2) terms.  All dense row-major; w2 is (n2, n1) with
 * contiguous rows, w3 has n2 elements.
 * Admitted: n1 == 256, n2 == 128, embed a multiple of 16 in 16 .. 128, num_users, num_items < 2^31; anything else is
 * CTR_ELIMIT.  A null pointer, a negative count, ldo < num_items, row_blocks < 0 or a row range outside the user table
 * is CTR_EINVAL; zu / zi / su / si / w2 not 16-byte aligned is CTR_EALIGN -- all before anything is enqueued.
 * rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.  Columns past num_items of a row of out are not
 * touched.  A workgroup takes CTR_DEEPFM_GRID_ITEM_TILE items and walks user tiles of CTR_DEEPFM_GRID_USER_TILE rows;
 * row_blocks > 0 is the number of workgroups that share an item tile's user tiles, 0 leaves it to the launch (a small
 * multiple of the CU count in all).  The caller validates `users`: an id outside [0, num_users) is clamped into the
 * table, not reported.  No atomics; a pair's score is a function of its user's rows, its item's rows and the weights
 * alone, bitwise, whatever the rows, their order, the items' positions or row_blocks. */
#define CTR_DEEPFM_GRID_ITEM_TILE 128
#define CTR_DEEPFM_GRID_USER_TILE 16
int ctr_deepfm_grid_scores(const float* zu, const float* zi, const float* su, const float* si, const float* a,
                           const float* b, int64_t num_users, int64_t num_items, int embed, int n1, int n2,
                           const float* w2, const float* b2, const float* w3, const float* b3, const float* out_w,
                           const float* out_b, const int64_t* users /*nullable*/, int64_t user0, int64_t rows,
                           float* out, int64_t ldo, int row_blocks, void* stream);

/* PNN (inner mode, six fields) over the user x item grid (csrc/pnn_grid.hip): the scores of `rows` users against EVERY
 * item in one launch, with no feature matrix.  Every field vector belongs to the user (fields 0, 2, 3, 4) or to the item
 * (1, 5) and the product layer's output has no activation, so the model splits into table rows the caller makes with
 * ctr_embed_fwd, ctr_allpairs_fwd and ctr_linear_fwd:
 *   z1 = zu[u_r] + zi[i] + g d(u_r, i)                                         (n1 = 128 wide; g is (n1, 8))
 *   d  = (<U0, I0>, <U0, I1>, <I0, U1>, <I0, U2>, <I0, U3>, <U1, I1>, <U2, I1>, <U3, I1>)   the eight cross products, in
 *        the column order of ctr_allpairs_fwd; U0..U3 = fu[u_r] (user, age, gender, occupation vectors, `embed` floats
 *        each), I0, I1 = fi[i] (item, movie vectors)
 *   out[r * ldo + i] = sigmoid(out_w . relu(d3_w relu(d2_w relu(z1) + d2_b) + d3_b) + out_b[0])    (n1 -> n2 = 64 -> n3 = 32)
 *   u_r = users[r] (users set: any order, repeats allowed) or user0 + r (users NULL; user0 + rows <= num_users)
 * zu (num_users, n1) / zi (num_items, n1): the first DNN layer applied to a side's part of the product layer's output
 * (the biases on the item side); fu (num_users, 4 embed), fi (num_items, 2 embed); g = d1_w W2[:, cross columns].  All
 * dense row-major; d2_w is (n2, n1), d3_w (n3, n2) with contiguous rows, out_w has n3 elements.
 * Admitted: n1 == 128, n2 == 64, n3 == 32, embed a multiple of 16 in 16 .. 256, num_users, num_items < 2^31; anything
 * else is CTR_ELIMIT.  A null pointer, a negative count, ldo < num_items, row_blocks < 0 or a row range outside the user
 * table is CTR_EINVAL; zu / zi / fu / fi / d2_w / d3_w not 16-byte aligned is CTR_EALIGN -- all before anything is
 * enqueued.  rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.  Columns past num_items of a row of out
 * are not touched.  A workgroup takes CTR_PNN_GRID_ITEM_TILE items and walks user tiles of CTR_PNN_GRID_USER_TILE rows;
 * row_blocks > 0 is the number of workgroups that share an item tile's user tiles, 0 leaves it to the launch (a small
 * multiple of the CU count in all).  The caller validates `users`: an id outside [0, num_users) is clamped into the
 * table, not reported.  No atomics; a pair's score is a function of its user's rows, its item's rows and the weights
 * alone, bitwise, whatever the rows, their order, the items' positions or row_blocks. */
#define CTR_PNN_GRID_ITEM_TILE 128
#define CTR_PNN_GRID_USER_TILE 16
int ctr_pnn_grid_scores(const float* zu, const float* zi, const float* fu, const float* fi, const float* g,
                        int64_t num_users, int64_t num_items, int embed, int n1, int n2, int n3, const float* d2_w,
                        const float* d2_b, const float* d3_w, const float* d3_b, const float* out_w, const float* out_b,
                        const int64_t* users /*nullable*/, int64_t user0, int64_t rows, float* out, int64_t ldo,
                        int row_blocks, void* stream);

/* AFM (six fields) over the user x item grid (csrc/afm_grid.hip): the scores of `rows` users against EVERY item in one
 * launch, with no feature matrix.  Every field vector belongs to the user (fields 0, 2, 3, 4) or to the item (1, 5), and
 * per pair product p the model needs only s(p) = att_h . relu(att_w^T p + att_b) and t(p) = out_w . p, so it splits into
 * table rows the caller makes with ctr_embed_fwd, ctr_pairprod_fwd and ctr_linear_fwd:
 *   (s_c, t_c) of the eight cross products U0 I0, U0 I1, U1 I0, U1 I1, U2 I0, U2 I1, U3 I0, U3 I1 (elementwise);
 *        U0..U3 = fu[u_r] (user, age, gender, occupation vectors, `embed` floats each), I0, I1 = fi[i] (item, movie)
 *   w = softmax over the 15 logits: the user's six (summarised by mU = max s, dU = sum exp(s - mU), nU = sum exp(s - mU) t),
 *        the item's one (sI, tI) and the eight s_c; the maximum runs along, so logits of any size are taken
 *   out[r * ldo + i] = sigmoid(a[u_r] + b[i] + sum_k w_k t_k)
 *   u_r = users[r] (users set: any order, repeats allowed) or user0 + r (users NULL; user0 + rows <= num_users)
 * su (num_users, 4): a, mU, dU, nU per user; si (num_items, 3): b, sI, tI per item (b holds every bias); fu (num_users,
 * 4 embed), fi (num_items, 2 embed); att_w is (embed, attention) as the model stores it, att_b and att_h have
 * `attention` elements, out_w `embed`.  All dense row-major.
 * Admitted: attention == 64, embed a multiple of 16 in 16 .. 128, num_users, num_items < 2^31; anything else is
 * CTR_ELIMIT.  A null pointer, a negative count, ldo < num_items, row_blocks < 0 or a row range outside the user table
 * is CTR_EINVAL; su / fu / fi / att_w not 16-byte aligned is CTR_EALIGN -- all before anything is enqueued, in that
 * order.  rows == 0 or num_items == 0 enqueues nothing and returns CTR_OK.  Columns past num_items of a row of out are
 * not touched.  A workgroup takes CTR_AFM_GRID_ITEM_TILE items and walks user tiles of CTR_AFM_GRID_USER_TILE rows;
 * row_blocks > 0 is the number of workgroups that share an item tile's user tiles, 0 leaves it to the launch (a small
 * multiple of the CU count in all).  The caller validates `users`: an id outside [0, num_users) is clamped into the
 * table, not reported.  No atomics; a pair's score is a function of its user's rows, its item's rows and the weights
 * alone, bitwise, whatever the rows, their order, the items' positions or row_blocks. */
#define CTR_AFM_GRID_ITEM_TILE 128
#define CTR_AFM_GRID_USER_TILE 16
int ctr_afm_grid_scores(const float* su, const float* si, const float* fu, const float* fi, int64_t num_users,
                        int64_t num_items, int embed, int attention, const float* att_w, const float* att_b,
                        const float* att_h, const float* out_w, const int64_t* users /*nullable*/, int64_t user0,
                        int64_t rows, float* out, int64_t ldo, int row_blocks, void* stream);

/* A biased low-rank product over the user x item grid (csrc/lowrank_grid.hip): the grid of MatrixFactorization, FFM and
 * LogisticRegression, the scores of `rows` users against EVERY item in one launch:
 *   out[r * ldo + i] = sigmoid((a[u_r] + b[i]) + sum_k cu[u_r * rank + k] ci[i * rank + k])
 *   u_r = users[r] (users set: any order, repeats allowed) or user0 + r (users NULL; user0 + rows <= num_users)
 * cu (num_users, rank) / ci (num_items, rank) dense row-major; a (num_users) / b (num_items) nullable: NULL is zeros.
 * rank == 0 takes cu == ci == NULL and needs a or b.  The dot is ONE chain per pair on v_mfma_f32_32x32x2_f32 (exact
 * f32, k ascending), then (a + b) + dot, then the sigmoid.  Admitted: rank 0 and every multiple of 16 up to 256,
 * num_users and num_items < 2^31; anything else is CTR_ELIMIT.  A null pointer (cu or ci at rank != 0, both biases at
 * rank 0, out), a negative count, ldo < num_items, row_blocks < 0 or a row range outside the user table is CTR_EINVAL;
 * cu / ci not 16-byte aligned is CTR_EALIGN -- all before anything is enqueued, in that order.  rows == 0 or
 * num_items == 0 enqueues nothing and returns CTR_OK.  Columns past num_items of a row of out are not touched.  A
 * workgroup takes CTR_LOWRANK_GRID_ITEM_TILE items (a wave 32 of them) and walks user tiles of
 * CTR_LOWRANK_GRID_USER_TILE rows: a wave's store instruction writes 128 contiguous bytes of two score rows.
 * row_blocks > 0 is the number of workgroups that share an item tile's user tiles, 0 leaves it to the launch.  The
 * caller validates `users`: an id outside [0, num_users) is clamped into the table, not reported.  No atomics; a pair's
 * score is a function of its user's row, its item's row and the two biases alone, bitwise, whatever the rows, their
 * order, the items' positions, ldo or row_blocks. */
#define CTR_LOWRANK_GRID_ITEM_TILE 128
#define CTR_LOWRANK_GRID_USER_TILE 32
int ctr_lowrank_grid_scores(const float* cu /*nullable*/, const float* ci /*nullable*/, const float* a /*nullable*/,
                            const float* b /*nullable*/, int64_t num_users, int64_t num_items, int rank,
                            const int64_t* users /*nullable*/, int64_t user0, int64_t rows, float* out, int64_t ldo,
                            int row_blocks, void* stream);

/* Wide & Deep over the user x item grid (csrc/deepfm_grid.hip): ctr_deepfm_grid_scores without its FM dot -- the same
 * kernel template, su / si and their stage compiled out:
 *   out[r * ldo + i] = sigmoid(out_w[0] (a[u_r] + b[i]) + out_w[1] relu(w3 . relu(w2 relu(zu[u_r] + zi[i]) + b2) + b3[0])
 *                              + out_b[0])
 * Arguments, refusals (n1 == 256 and n2 == 128 only; zu / zi / w2 16-byte aligned), tiles and the bitwise contract as
 * there. */
#define CTR_WIDEDEEP_GRID_ITEM_TILE 128
#define CTR_WIDEDEEP_GRID_USER_TILE 16
int ctr_widedeep_grid_scores(const float* zu, const float* zi, const float* a, const float* b, int64_t num_users,
                             int64_t num_items, int n1, int n2, const float* w2, const float* b2, const float* w3,
                             const float* b3, const float* out_w, const float* out_b, const int64_t* users /*nullable*/,
                             int64_t user0, int64_t rows, float* out, int64_t ldo, int row_blocks, void* stream);

/* gy: gradient of the LAST layer's output; gx (nullable): gradient of x.  workspace is
 * required: (number of workgroups <= 256) * sum_i (n_i*k_i + n_i) floats. */
int ctr_mlp_bwd(const float* x, int64_t ldx, int64_t m, const ctr_mlp_layer_t* layers, int nlayers,
                const float* gy, int64_t ldgy, float* gx, int64_t ldgx,
                float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------
 * Row-sharded tables across the GPUs of a node (no counterpart in the reference,
 * which is single-device): owner(row) = row % world, local
 * row = row / world.  Buckets `n` global ids by owner ahead of the RCCL all-to-all:
 *   counts[w]  = ids owned by rank w, w < world; counts[world] = ids outside [0, vocab)  (world + 1 int64, written)
 *   send[slot] = local row as int32 (the wire format), buckets back to back in rank order
 *   perm[i]    = slot of id i;  inv[slot] = i           (order inside a bucket is not fixed)
 * cursor: CTR_SHARD_SCRATCH_INT64(world) int64 of scratch (per-workgroup histograms; no global atomics are used).
 * Ids outside [0, vocab) travel as row 0 and are counted.
 * ---------------------------------------------------------------------- */
#define CTR_SHARD_SCRATCH_INT64(world) (256 * ((world) + 1))
int ctr_shard_bucket(const int64_t* ids, int64_t n, int world, int64_t vocab, int64_t* counts, int64_t* cursor,
                     int32_t* send, int64_t* perm, int64_t* inv, void* stream);
/* The capacity-bounded layout of the same bucketing: bucket w is slots [w*cap, (w+1)*cap) of `send` / `inv`
 * (world*cap entries each) whatever the counts are, so the all-to-all has equal, host-known splits and a fresh id
 * tensor needs no host read before its ids travel.  send[slot] = local row or -1 (unused); perm[i] = slot of id i;
 * inv[slot] = i (an unused slot names some id of the batch: its row is masked out by the owner).  cursor:
 * CTR_SHARD_SCRATCH_INT64(world) int64 of scratch.
 * state (4 int64, written): {1 if a bucket received more than cap ids -- those ids are NOT placed, the caller must
 * fall back to ctr_shard_bucket --, ids outside [0, vocab), n, -n}: MAX-all-reduced by the caller. */
int ctr_shard_bucket_padded(const int64_t* ids, int64_t n, int world, int64_t vocab, int64_t cap, int64_t* cursor,
                            int32_t* send, int64_t* perm, int64_t* inv, int64_t* state, void* stream);
/* owner side of the padded exchange: rows[j] = recv[j] if it is a row of this shard, else j % local_rows (a harmless
 * target: the slot's gradient row is multiplied by valid[j] = 0); valid[j] = 1.0 / 0.0; mark[j] = recv[j] or -1 (what
 * ctr_rows_mark skips) */
int ctr_shard_recv_rows(const int32_t* recv, int64_t slots, int64_t local_rows, int64_t* rows, float* valid,
                        int64_t* mark, void* stream);
/* table[idx[i]][0:dim] = 0 for i < n (idx outside [0, rows) skipped): clears the rows one step touched in a
 * persistent dense shard-gradient buffer instead of zero-filling the whole shard */
int ctr_rows_zero(float* table, int64_t ld, int64_t rows, int dim, const int64_t* idx, int64_t n, void* stream);

/* Gradient of two (V, 1) first-order tables indexed by the float id columns `user_col` / `item_col` of the (B, ldx)
 * feature matrix (model/ffm.py:19-26 `user` / `item` embeddings, lr.py / widedeep.py / deepfm.py first-order terms):
 * guser1[x[b, user_col]] += v_b, gitem1[x[b, item_col]] += v_b with v_b = g[b*ldg], or g[b*ldg] * p (1 - p) with
 * p = prob[b*ldp] when prob is not NULL (the dlogit of a sigmoid head).  Ids outside their table are skipped.  Either
 * gradient may be NULL.  Small tables only (num_users + num_items <= CTR_ROWS1_MAX_ROWS: they are summed in LDS per
 * workgroup; CTR_ELIMIT beyond -- the interaction kernels' own first-order atomics are the path for large tables). */
#define CTR_ROWS1_MAX_ROWS 32768
int ctr_rows1_scatter(const float* x, int64_t ldx, int user_col, int item_col, const float* g, int64_t ldg,
                      const float* prob, int64_t ldp, int64_t batch, float* guser1, int64_t num_users, float* gitem1,
                      int64_t num_items, void* stream);

/* ------------------------------------------------------------------------
 * Ranking step of recommendation() (model/mf.py:28-35, neuralcf.py:61-72, pnn.py:133-143, din.py:55-66: torch.topk
 * over one user's candidate scores): for each of `rows` rows of n scores (element (r, j) at
 * scores[r*row_stride + j*col_stride]) the indices of the k best, best first.  Order: score descending, NaN first
 * (torch's convention), equal scores by ascending index (fixed, where torch leaves ties unspecified).
 * idx_out (rows, k) int64; val_out (rows, k) nullable.  k <= 4096 (CTR_ELIMIT beyond), k <= n < 2^31.
 * ---------------------------------------------------------------------- */
#define CTR_TOPK_MAX_K 4096
int ctr_topk_rows(const float* scores, int64_t row_stride, int64_t col_stride, int64_t rows, int64_t n, int k,
                  int64_t* idx_out, float* val_out, void* stream);

/* ------------------------------------------------------------------------
 * Neighbourhood collaborative filtering (UserCF_Final.py / ItemCF_Final.py), on an int8 0/1 matrix x
 * (rows x cols_pad, row-major, cols_pad % 64 == 0, zero padded, 16-byte aligned) and its int32 row counts.
 *
 * ctr_cf_knn replaces cosine_similarity(data) (UserCF_Final.py:23) / cosine_similarity(data.T) (ItemCF_Final.py:22)
 * and the per-row sort of recommendations_list (UserCF_Final.py:51-53) / prediction_item_based (ItemCF_Final.py:30-33):
 * for each query row q in [q_begin, q_begin + q_count) the kk best rows of all `rows` by
 *   sim = float32(c / sqrt(a b)) evaluated in double (0 when a or b is 0), c = intersection count, a, b = row counts,
 * descending, ties by ascending index; q itself included (the caller drops position 0 as the reference does).
 * idx_out / sim_out (q_count, kk) int64 / float32; a list shorter than kk (rows < kk) ends in -1 / 0.
 * The rows x rows similarity is never written.  kk <= CTR_CF_KNN_MAX_K (CTR_ELIMIT beyond), rows < 2^31.
 *
 * ctr_usercf_scores (prediction_dating, UserCF_Final.py:26-39): out[b, i] = sum_j s_j x[v_j, i] / sum_j s_j over the
 * k neighbours v_j = nbr[u k + j], s_j = nsim[u k + j] of u = users[b] (index -1: no neighbour), float32 accumulated in
 * neighbour order, 0 when the denominator is 0, -inf where x[u, i] != 0 (rated) or u is outside [0, num_users).
 * ctr_itemcf_scores (prediction_item_based, ItemCF_Final.py:27-38): out[b, i] = sum_j s_ij x[u, j] / sum_j s_ij over
 * the k neighbours j = nbr[i k + ..] of item i, same conventions.  cols_pad / 8 <= 65536 (CTR_ELIMIT beyond).
 * out (batch, ldo) float32, ldo >= num_items; items i < num_items <= cols_pad written.
 * ---------------------------------------------------------------------- */
#define CTR_CF_KNN_MAX_K 64
int ctr_cf_knn(const int8_t* x, int64_t rows, int64_t cols_pad, const int32_t* counts, int64_t q_begin,
               int64_t q_count, int kk, int64_t* idx_out, float* sim_out, void* stream);
int ctr_usercf_scores(const int8_t* x, int64_t num_users, int64_t cols_pad, int64_t num_items, const int64_t* nbr,
                      const float* nsim, int k, const int64_t* users, int64_t batch, float* out, int64_t ldo,
                      void* stream);
int ctr_itemcf_scores(const int8_t* x, int64_t num_users, int64_t cols_pad, int64_t num_items, const int64_t* nbr,
                      const float* nsim, int k, const int64_t* users, int64_t batch, float* out, int64_t ldo,
                      void* stream);

/* ------------------------------------------------------------------------
 * GDCF (GDCF_Final.py): matrix factorisation on the full implicit matrix.  BCEWithLogitsLoss, mean reduction, over
 * all m x n entries of the 0/1 matrix Y (m = num_users, n = num_items) with scores S = P Q^T:
 *   loss = sum_{u,i} (softplus(s_ui) - y_ui s_ui) / (m n),  G = sigmoid(S) - Y,  dP = G Q / (m n),  dQ = G^T P / (m n).
 * p (m, k) and q (n, k) float32 row-major with leading dimension k; 1 <= k <= CTR_GDCF_MAX_DIM (CTR_ELIMIT beyond).
 * The m x n scores are never written: two fused fp32 matrix-core passes, 1/(m n) evaluated in double, no atomics, so
 * every output is bitwise reproducible.  Padding columns of the int8 matrices (>= num_items, resp. >= num_users) are
 * excluded from the loss and the gradients.
 *
 * ctr_gdcf_rows (the forward): *loss (device float32) and, when grad_p is not NULL, grad_p (m, k) = dP.  y is the
 * (m, ldy) int8 matrix, ldy % 64 == 0, ldy >= n, 16-byte aligned.  workspace: device memory of at least
 * ctr_gdcf_workspace_bytes(m, n, k) bytes (float64 partials of the loss).
 * ctr_gdcf_cols (the backward of q): grad_q (n, k) = gout[0] * dQ with gout a device float32 (the upstream gradient
 * of the loss).  yt is the transposed (n, ldyt) int8 matrix, ldyt % 64 == 0, ldyt >= m, 16-byte aligned.
 * ---------------------------------------------------------------------- */
#define CTR_GDCF_MAX_DIM 256
int ctr_gdcf_workspace_bytes(int64_t num_users, int64_t num_items, int k, int64_t* bytes /*host, out*/);
int ctr_gdcf_rows(const float* p, const float* q, int64_t num_users, int64_t num_items, int k, const int8_t* y,
                  int64_t ldy, float* loss, float* grad_p, void* workspace, int64_t workspace_bytes, void* stream);
int ctr_gdcf_cols(const float* p, const float* q, int64_t num_users, int64_t num_items, int k, const int8_t* yt,
                  int64_t ldyt, const float* gout, float* grad_q, void* stream);

/* ------------------------------------------------------------------------
 * Full softmax over the catalogue: the cross entropy of a target item against every item.  For query rows x
 * (batch, k), an item table q (num_items, k) (both float32 row-major, leading dimension k) and target (batch) int64:
 *   z[b, i] = <x[b], q[i]>,  lse[b] = log sum_i exp(z[b, i]),  nll[b] = lse[b] - z[b, t_b],
 *   G[b, i] = gout[b] (exp(z[b, i] - lse[b]) - [i == t_b]),  dX = G q,  dQ = G^T x.
 * No temperature, no item bias, no exclusion.  The batch x num_items logits are never written: two fused fp32
 * matrix-core passes (running maximum: exp never sees a positive argument), no atomics, so every output is bitwise
 * reproducible.  1 <= k <= CTR_SOFTMAX_FULL_MAX_DIM, batch and num_items < 2^31, splits <= 64 (CTR_ELIMIT beyond).
 * A target outside [0, num_items) is never dereferenced: that row has no indicator term, nll = lse, and *err_flag
 * (device int32, may be NULL) is set to 1.  An empty batch is CTR_OK and enqueues nothing.
 *
 * splits: into how many parts a pass cuts the range it streams (items for the rows, batch rows for the columns) so
 * that small shapes fill the device; 0: chosen from (batch, num_items, k) and the CU count.  With more than one part
 * the partials go to `workspace` (device, at least ctr_softmax_full_workspace_bytes for these splits; 1 needs none)
 * and a second launch merges them in ascending part order.
 * ctr_softmax_full_rows: nll and lse (batch) and, when grad_x is not NULL, grad_x (batch, k) = dX for gout = 1:
 *   softmax(z[b]) q - q[t_b]; the caller scales it by its upstream gradient.
 * ctr_softmax_full_cols: grad_q (num_items, k) = dQ from the lse of the row pass and gout (batch) float32.  nll (may be
 *   NULL): the row pass's nll; with it a target's entry is gout expm1(-nll), exact where its probability nears 1 (a
 *   float32 lse alone leaves it an error of half an ulp of lse there).
 * ---------------------------------------------------------------------- */
#define CTR_SOFTMAX_FULL_MAX_DIM 256
int ctr_softmax_full_workspace_bytes(int64_t batch, int64_t num_items, int k, int splits_rows, int splits_cols,
                                     int64_t* bytes /*host, out*/);
int ctr_softmax_full_rows(const float* x, const float* q, int64_t batch, int64_t num_items, int k,
                          const int64_t* target, float* nll, float* lse, float* grad_x, int splits, void* workspace,
                          int64_t workspace_bytes, int32_t* err_flag, void* stream);
int ctr_softmax_full_cols(const float* x, const float* q, int64_t batch, int64_t num_items, int k,
                          const int64_t* target, const float* lse, const float* nll, const float* gout, float* grad_q,
                          int splits, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * ALS: implicit-feedback matrix factorisation by alternating least squares (Hu, Koren & Volinsky 2008).  With the
 * other table y (y_rows, k) fixed (float32 row-major, leading dimension k, 16-byte aligned) and gram = y^T y, row u of
 * a CSR (indptr (csr_rows + 1) int64, indices int32 rows of y, both on the device) gets the solution of
 *   (gram + alpha * sum_{i in N(u)} y_i y_i^T + reg I) x_u = (1 + alpha) * sum_{i in N(u)} y_i,
 * the minimiser of sum_i c_ui (p_ui - <x_u, y_i>)^2 + reg |x_u|^2 over ALL rows i of y with c = 1 + alpha on the
 * listed rows (p = 1) and c = 1 elsewhere (p = 0).  An empty list gives exact zeros.
 * k a multiple of 16 in [16, CTR_ALS_MAX_DIM], rows, y_rows and count < 2^31 (CTR_ELIMIT beyond).
 *
 * ctr_als_gram: gram (k, k) = y^T y, full and symmetric.  Partials over fixed slabs of rows go to `workspace` (device,
 *   at least ctr_als_gram_workspace_bytes) and a second launch adds them in ascending slab order: no atomics, the
 *   result is bitwise reproducible.
 * ctr_als_solve_rows: out[j] (count rows, leading dimension ldo >= k) = x of CSR row rows[j] (rows NULL: row j).  One
 *   workgroup per row: the k x k system is assembled on the fp32 matrix cores, factorised (Cholesky) and solved in
 *   LDS; no workspace, no (count, k, k) tensor.  A result is a bitwise function of the row's list, y, gram, reg and
 *   alpha alone -- not of which rows are asked for, in what order or how often.  Guards through *err_flag (device
 *   int32, may be NULL, OR-ed into, never cleared): an index outside [0, y_rows), a row id outside [0, csr_rows) or a
 *   row with indptr[u + 1] < indptr[u] is never dereferenced, sets bit 1 and that out row is zeros (the CSR is
 *   otherwise trusted: the call carries no nnz, so offsets past the end of `indices` cannot be told); a pivot that
 *   is not a positive finite number (reg = 0 on a singular system, a NaN in y) or a non-finite result sets bit 2 and
 *   that out row is zeros.  No NaN or Inf is ever stored.  count == 0 is CTR_OK and enqueues nothing; a null pointer or a bad size is CTR_EINVAL before a launch.
 * ---------------------------------------------------------------------- */
#define CTR_ALS_MAX_DIM 128
int ctr_als_gram_workspace_bytes(int64_t rows, int k, int64_t* bytes /*host, out*/);
int ctr_als_gram(const float* y, int64_t rows, int k, float* gram, void* workspace, int64_t workspace_bytes,
                 void* stream);
int ctr_als_solve_rows(const float* y, int64_t y_rows, int k, const float* gram, const int64_t* indptr,
                       const int32_t* indices, int64_t csr_rows, const int64_t* rows /* NULL: 0 .. count-1 */,
                       int64_t count, float reg, float alpha, float* out, int64_t ldo, int32_t* err_flag, void* stream);

/* ctr_als_solve_rows_weighted: the same row solve with a weight per list entry.  values (nnz float32, device) is
 * aligned with indices; entry e of a row of n entries counts with w_e = fmaf(w1, v_e, w0) and t_e = fmaf(t1, v_e, t0):
 *   (G + sum_e w_e y_e y_e^T + (reg + reg_per_entry * n) I) x = sum_e t_e y_e,      G = gram, or 0 when gram is NULL.
 *   confidences c = 1 + alpha v (Hu et al.):  gram,  (w0, w1, t0, t1) = (0, alpha, 1, alpha),  reg
 *   explicit ratings, weighted-lambda (Zhou et al. 2008):  gram NULL,  (1, 0, 0, 1),  reg_per_entry
 *   the unit system above, with v = 1:  gram,  (alpha, 0, 1 + alpha, 0),  reg   (not bitwise ctr_als_solve_rows)
 * Arguments, limits, the one-workgroup-per-row frame, the guards and the meaning of the err_flag bits are those of
 * ctr_als_solve_rows.  A row is a bitwise function of its list, its values, y, gram and the six scalars alone.
 * Nothing at or past indptr[u + 1] is read, neither an index nor a value.  A non-finite value or scalar reaches the
 * pivot / finite guard: bit 2 and a zero row, no NaN or Inf is stored.  A negative w_e is the caller's business; an
 * indefinite system is caught by the pivot guard.  An empty list gives exact zeros whatever the scalars are.
 * Refusals before a launch: CTR_EINVAL for values NULL where indices is not (indices NULL: a CSR without a pair), a
 * NaN scalar, ldo < k or a null y / indptr / out; CTR_ELIMIT for k; count == 0 is CTR_OK and enqueues nothing. */
int ctr_als_solve_rows_weighted(const float* y, int64_t y_rows, int k, const float* gram /* NULL: no dense part */,
                                const int64_t* indptr, const int32_t* indices, const float* values, int64_t csr_rows,
                                const int64_t* rows /* NULL: 0 .. count-1 */, int64_t count, float w0, float w1,
                                float t0, float t1, float reg, float reg_per_entry, float* out, int64_t ldo,
                                int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------------
 * Graph propagation (LightGCN, He et al. 2020): a sparse-times-dense row sum over a CSR.  For every requested row
 *   out[j, :] = s_out[r] * sum_{e in [indptr[r], indptr[r+1])} s_in[indices[e]] * x[indices[e], :],    r = rows[j]
 * x (x_rows, k) float32 with leading dimension ldx; indptr (num_rows + 1) int64 and indices (nnz) int32 as the other
 * CSR entries take them; s_in (x_rows) and s_out (num_rows) float32, either NULL: ones; rows (count) int64, NULL: the
 * rows 0 .. count-1; out (count, k) with leading dimension ldo.  k a multiple of 16 in [16, CTR_GRAPH_MAX_DIM];
 * x_rows, num_rows, nnz, count, nwork and nmerge < 2^31 (CTR_ELIMIT beyond); x, out and workspace 16-byte aligned, ldx
 * and ldo multiples of 4 (CTR_EALIGN otherwise).
 *
 * One wave sums one work item in registers, 16-byte loads per lane, the source scale read per entry and applied by one
 * fused multiply-add; a lane without an entry adds nothing.  A list is cut every CTR_GRAPH_SEGMENT entries counted
 * from its own start; segment sums are added in ascending segment order and the total is scaled once.  There is no
 * float atomic, and out[j] is a bitwise function of the row's list, the source rows it names and the two scales -- not
 * of which rows are asked for, of their order, of the plan, of the launch geometry or of the run.  An empty list gives
 * exact zeros.  Source rows that no list names are never read.
 *
 * The plan (all of it optional, device memory, built once per CSR by the caller):
 *   work  (nwork, 4) int32: (out row j, segment s, workspace slot, 0).  slot < 0: the wave walks the whole row and
 *         writes out[j]; slot >= 0: the wave sums segment s alone into slot `slot` of the workspace (k floats a slot).
 *         NULL (nwork = 0): every out row is one whole-row item.  Items run in the order given: longest rows first.
 *   merge (nmerge, 2) int32: (out row j, first slot): out[j] = s_out * (slot + slot+1 + ...), one slot per segment of
 *         the row, in a second launch.  Every row whose items carry slots must be listed here once.
 *   workspace: at least ctr_graph_propagate_workspace_bytes(slots, k) bytes; may be NULL where nmerge == 0.
 * Guards through *err_flag (device int32, may be NULL, OR-ed into, never cleared), none of which traps: an index
 * outside [0, x_rows) is never dereferenced, adds nothing and sets bit 1, other rows are unaffected; a row id outside
 * [0, num_rows) or offsets that run backwards or past nnz give a zero row and bit 1; a work or merge item that names
 * an out row outside [0, count) or slots outside the workspace is skipped and sets bit 2.
 * Refusals before a launch: CTR_EINVAL for a null x / indptr / out, indices NULL with nnz > 0, a negative size,
 * ldx < k or ldo < k, work or merge NULL with a non-zero length (or the reverse), nmerge > 0 without work and
 * workspace; then CTR_ELIMIT; then CTR_EALIGN.  count == 0 is CTR_OK and enqueues nothing.
 * ---------------------------------------------------------------------- */
#define CTR_GRAPH_MAX_DIM 256
#define CTR_GRAPH_SEGMENT 512
int ctr_graph_propagate_workspace_bytes(int64_t partials, int k, int64_t* bytes /*host, out*/);
int ctr_graph_propagate(const float* x, int64_t x_rows, int64_t ldx, int k, const int64_t* indptr,
                        const int32_t* indices, int64_t num_rows, int64_t nnz, const float* s_in /* NULL: ones */,
                        const float* s_out /* NULL: ones */, const int64_t* rows /* NULL: 0 .. count-1 */,
                        int64_t count, const int32_t* work, int64_t nwork, const int32_t* merge, int64_t nmerge,
                        float* out, int64_t ldo, void* workspace, int64_t workspace_bytes, int32_t* err_flag,
                        void* stream);

/* ------------------------------------------------------------------------
 * Top-k ranking evaluation (evaluator/ranking.py: Ranking, and data/reader.py:137-159: remove_itemid).
 *
 * Id sets are CSRs over `rows` users: off (rows + 1, absolute into ids, device), ids (nnz, ascending within a row,
 * device).  Offsets live on the device, so their consistency is checked there: a row with off[u] < 0,
 * off[u+1] < off[u] or off[u+1] > nnz is read as empty and ORs CTR_RANK_ERR_OFFSETS into *err_flag (device int32,
 * zeroed by the caller).  The per-user results are written as a (rows, 7) float64 row of partials
 *   same = |set(a) & set(p[:k])|, rec = |set(p[:k])|, real = |set(a)|,
 *   ap   = sum_{i<k, p[i] in a} hits_i / (i + 1) / alen[u]       (ranking.py:43-63, alen = len(a) as given),
 *   dcg  = sum_{j<k, p[j] in a} 1 / log2(j + 2),  idcg = the same sum over min(k, sum_j [p[j] in a]) leading ones
 *          (ranking.py:76-110: r over the whole p),
 *   rr   = 1 / (j + 1) for the first p[j] in a over the whole p, else 0 (ranking.py:122-132);
 * -1 is an ordinary id throughout, as in the reference.  The aggregate (ranking.py:11-41, 65-74, 112-120, 134-141)
 * is a fixed-order host reduction of the partials.
 *
 * ctr_rank_filter (remove_itemid): out[u, :out_len[u]] = the entries of rec[u, :len] not in exclusion row u, in
 * order.  out may have ld_out >= len; entries past out_len[u] are not written.
 * ctr_rank_metrics_lists (Ranking on explicit rows): p = pred[u, :pred_len[u]] (pred_len NULL: len), a = the sorted
 * CSR row u of the actual ids (every entry, pads included), alen[u] its original length.  table: int64 workspace of
 * table_slots >= ctr_rank_table_slots(k, len) slots (more slots run more users at once); ids must not be INT64_MIN.
 * ctr_rank_mask: scores[u, id] = bits CTR_RANK_MASK_BITS for every id in [0, n) of exclusion row u.  That float is the
 * lowest key of ctr_topk_rows' order, below -inf and every other NaN.
 * ctr_rank_metrics_scores (Ranking(a, remove_itemid(..(topk_rows(s, n))..)) without the full ranking): row u of the
 * masked scores has n_real[u] survivors; p = the survivors in ctr_topk_rows' order followed by pad[u] times -1.
 * topk (rows, kt), kt = min(k, n), is ctr_topk_rows of the masked rows.  The first hit of MRR comes from one pass over
 * the row: the survivors ordered above the best relevant one.  A survivor that is NaN or -inf ORs
 * CTR_RANK_ERR_SURVIVOR, a survivor count other than n_real[u] CTR_RANK_ERR_COUNT, n_real or pad out of range
 * CTR_RANK_ERR_LENGTH (then the row is treated as empty); the partials of such a row are not meaningful.
 * k >= 1 (CTR_EINVAL otherwise); rows <= CTR_RANK_MAX_ROWS (CTR_ELIMIT beyond).
 * ---------------------------------------------------------------------- */
#define CTR_RANK_MAX_ROWS (1ll << 24)
#define CTR_RANK_MASK_BITS 0xffffffffu
#define CTR_RANK_ERR_OFFSETS 1
#define CTR_RANK_ERR_LENGTH 2
#define CTR_RANK_ERR_SURVIVOR 4
#define CTR_RANK_ERR_COUNT 8
int ctr_rank_filter(const int64_t* rec, int64_t ld_rec, int64_t rows, int64_t len, const int64_t* ex_off,
                    const int64_t* ex_ids, int64_t ex_nnz, int64_t* out, int64_t ld_out, int64_t* out_len,
                    int32_t* err_flag, void* stream);
int ctr_rank_table_slots(int64_t k, int64_t len, int64_t* slots);   /* *slots (host) = smallest power of two
                                                                      >= max(64, 2 min(k, len)) */
int ctr_rank_metrics_lists(const int64_t* pred, int64_t ld_pred, const int64_t* pred_len, int64_t rows, int64_t len,
                           const int64_t* act_off, const int64_t* act_ids, int64_t act_nnz, const int64_t* alen,
                           int64_t k, int64_t* table, int64_t table_slots, double* partials, int32_t* err_flag,
                           void* stream);
int ctr_rank_mask(float* scores, int64_t ld, int64_t rows, int64_t n, const int64_t* ex_off, const int64_t* ex_ids,
                  int64_t ex_nnz, int32_t* err_flag, void* stream);
int ctr_rank_metrics_scores(const float* scores, int64_t ld, int64_t rows, int64_t n, const int64_t* topk, int64_t kt,
                            int64_t k, const int64_t* act_off, const int64_t* act_ids, int64_t act_nnz,
                            const int64_t* alen, const int64_t* n_real, const int64_t* pad, double* partials,
                            int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------------
 * The host work either side of the step, on the device.
 * ctr_negative_sample (sampler/sampler.py:16-48): for every user u < num_users, num_negatives items drawn
 * uniformly from [0, num_items), each redrawn while bit `item` of the user's row of `excluded`
 * (num_users x words_per_user uint32, bit i of word i/32 = pair (u, i) observed) is set.
 * users[u*num_negatives + j] = u, items[...] = the draw; counter-based generator: the sample depends on
 * `seed` only.  *fail_flag (nullable) is raised if a slot found no free item in 16384 draws.
 * ctr_assemble_features (data/reader.py:98-101): out[b, :] = [users[b], items[b] as floats,
 * user_feat[users[b], :user_width], item_feat[items[b], :item_width]] -- the (B, 45) matrix of the feature
 * models at user_width = 24 (age, 2 gender, 21 occupation columns), item_width = 19 (genre flags).
 * ---------------------------------------------------------------------- */
int ctr_negative_sample(const uint32_t* excluded, int64_t words_per_user, int64_t num_users, int64_t num_items,
                        int num_negatives, uint64_t seed, int64_t* users, int64_t* items, int32_t* fail_flag,
                        void* stream);
int ctr_assemble_features(const int64_t* users, const int64_t* items, int64_t n, const float* user_feat,
                          int user_width, int64_t num_users, const float* item_feat, int item_width,
                          int64_t num_items, float* out, int64_t ldo, int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------------
 * Mini-batch loader: one launch builds every tensor of one batch of a shuffled epoch.  (The reference trains
 * full-batch, trainer/trainer.py:23-40; its data/dataloader.py and data/dataset.py are empty.)
 * Position p of epoch e reads sample perm(seed, e, p): a keyed 4-round Feistel network with cycle walking,
 * defined in the header comment of csrc/loader.hip -- stateless, no permutation array, independent of the launch
 * geometry.  shuffle == 0 makes the index the identity.
 * The descriptor is a host struct, copied by value into the launch:
 *   cols      each (n, width) source of 4- or 8-byte elements (float32 / int64), row idx copied to row b of dst;
 *   feature   (feat_out non-null)  feat_out[b, :] = what ctr_assemble_features writes for
 *             (feat_users[idx], feat_items[idx]), the id columns as floats included;
 *   history   (hist_out non-null)  hist_out[b, :hist_len] = history[hist_users[idx], :hist_len].
 * An id of a join outside its table raises *err_flag (nullable) and reads row 0.
 * ctr_load_batch writes the batch of positions [first, first + count), first + count <= n.
 * ctr_loader_indices writes their sample indices to out (count int64): the permutation alone, for inspection.
 * count == 0 is a no-op; n < 1, a negative epoch or first, or a range beyond n is CTR_EINVAL.
 * ctr_load_batch_neg draws negatives inside the same launch: the epoch has n * (1 + negatives) positions, every
 * positive once and `negatives` drawn items per positive, none of them in the observed set (a CSR over users); the
 * definition stands in the header comment of csrc/loader.hip.  A negative is sample s with the drawn item in cols[item_col]
 * (and in the feature join) and 0.0f in cols[rating_col].  The position range is checked against n * (1 + negatives);
 * negatives < 1, a column index out of range or of the wrong width or element size, num_items < 1 or >= 2^31, or
 * n * (1 + negatives) > 2^62 is CTR_EINVAL.  *fail_flag is raised when 2^14 draws of one slot were all observed.
 * ctr_load_batch_groups is ctr_load_batch_neg with a grouped shuffle: same descriptors, arguments and refusals, and
 * with k = negatives position p of epoch e holds
 *     g = p / (1 + k);  j = p % (1 + k)
 *     s = perm_n(seed, e, g)          (the keyed permutation over n, not over n * (1 + k);  s = g when shuffle == 0)
 *     v = s * (1 + k) + j
 *     outputs = exactly what ctr_load_batch_neg defines for virtual index v
 *               (j == 0: positive s;  j >= 1: the draw keyed by (seed, e, v))
 * so a batch whose first and count are multiples of 1 + k is a run of whole groups, positive first: what the group
 * losses below (ctr_group_loss_fwd) read.  Unshuffled it equals ctr_load_batch_neg bit for bit; shuffled, an epoch
 * emits the same multiset of samples as ctr_load_batch_neg for the same (seed, e).
 * ---------------------------------------------------------------------- */
typedef struct ctr_loader_col {
  const void* src;      /* (n, width) elements, leading dimension lds */
  void* dst;            /* (count, width) elements, leading dimension ldd */
  int64_t lds;
  int64_t ldd;
  int32_t width;        /* >= 1 */
  int32_t elem_bytes;   /* 4 or 8 */
} ctr_loader_col_t;

typedef struct ctr_loader {
  int64_t n;                    /* samples */
  int32_t ncols;                /* <= CTR_MAX_FIELDS */
  int32_t reserved;
  ctr_loader_col_t cols[CTR_MAX_FIELDS];
  const int64_t* feat_users;    /* (n,) */
  const int64_t* feat_items;    /* (n,) */
  const float* user_feat;       /* (num_users, user_width) */
  const float* item_feat;       /* (num_items, item_width) */
  int64_t num_users;
  int64_t num_items;
  int32_t user_width;
  int32_t item_width;
  float* feat_out;              /* (count, 2 + user_width + item_width), NULL = no feature join */
  int64_t feat_ldo;
  const int64_t* hist_users;    /* (n,) */
  const int64_t* history;       /* (hist_rows, hist_len), leading dimension ld_history */
  int64_t hist_rows;
  int64_t hist_len;
  int64_t ld_history;
  int64_t* hist_out;            /* (count, hist_len), NULL = no history join */
  int64_t hist_ldo;
  int32_t* err_flag;            /* device int32, nullable */
} ctr_loader_t;

int ctr_load_batch(const ctr_loader_t* loader, uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle,
                   void* stream);
int ctr_loader_indices(int64_t n, uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle, int64_t* out,
                       void* stream);

typedef struct ctr_loader_neg {
  int32_t negatives;            /* k >= 1 */
  int32_t item_col;             /* index into cols[] of the int64 width-1 item column, or -1 (features family) */
  int32_t rating_col;           /* index into cols[] of the float32 width-1 rating column */
  int32_t reserved;
  const int64_t* users;         /* (n,) user id of every positive */
  int64_t num_users;
  int64_t num_items;
  const int64_t* indptr;        /* (num_users + 1) */
  const int32_t* indices;       /* sorted, distinct per row */
  int32_t* fail_flag;           /* device int32, nullable */
} ctr_loader_neg_t;

int ctr_load_batch_neg(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, uint64_t seed, int64_t epoch,
                       int64_t first, int64_t count, int shuffle, void* stream);
int ctr_load_batch_groups(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, uint64_t seed, int64_t epoch,
                          int64_t first, int64_t count, int shuffle, void* stream);

/* Weighted negatives: ctr_load_batch_neg_pop / ctr_load_batch_groups_pop are the two entry points above with the draw
 * taken from an alias table instead of uniformly (header comment of csrc/loader.hip): try t of slot v picks column
 * col = ((h >> 32) * num_items) >> 32 of the table with the same hash h and keeps it when (h & 0xffffffff) < thresh_col,
 * else takes alias_col; table[c] = (thresh_c << 32) | alias_c, a column that always keeps itself has alias_c == c.
 * The observed-set rule, the 2^14 tries, *fail_flag and the bad-user rule are unchanged.  ctr_loader_t and
 * ctr_loader_neg_t are passed as above.  When logq_out is set every position b also writes
 *     logq_out[b * logq_ldo] = log_q[item of the position]      (a positive: pos_items[s]; a negative: the drawn item)
 * a bitwise copy; an item id outside [0, num_items) raises *err_flag and writes 0.0f.  A null table, pos_items or log_q,
 * or a logq_out with logq_ldo < 1, is CTR_EINVAL; a table or pos_items off 8 bytes is CTR_EALIGN. */
typedef struct ctr_loader_pop {
  const uint64_t* table;        /* (num_items,) alias-table words */
  const int64_t* pos_items;     /* (n,) item id of every positive */
  const float* log_q;           /* (num_items,) log of the table's distribution */
  float* logq_out;              /* (count,) elements, stride logq_ldo; nullable */
  int64_t logq_ldo;
} ctr_loader_pop_t;

int ctr_load_batch_neg_pop(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, const ctr_loader_pop_t* pop,
                           uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle, void* stream);
int ctr_load_batch_groups_pop(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, const ctr_loader_pop_t* pop,
                              uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle, void* stream);

/* ------------------------------------------------------------------------
 * Sampled leave-one-out evaluation (csrc/group_eval.hip): every held-out positive is ranked against k sampled
 * negatives, "1 positive + 99 negatives, HR@10 / NDCG@10".
 * ctr_eval_candidates draws the candidates.  n positives (users[s], items[s]); the observed set is the loader's CSR
 * (indptr (num_users + 1) int64, indices (nnz) int32 ascending and distinct within a row).  cand is (n, 1 + k) int64
 * with leading dimension ld >= 1 + k; columns past 1 + k are not touched.  Row s:
 *   cand[s, 0]    = items[s]
 *   gseed_s       = mix64(seed ^ mix64(s * 0x100000001B3 + 5))
 *   q_t           = perm_{num_items}(gseed_s, 0, t),  t = 0 .. num_items - 1      (csrc/loader_perm.h)
 *   cand[s, 1..k] = the first k of q_0, q_1, .. that are neither items[s] nor observed for users[s], in that order
 * so the k negatives are distinct and the draw with k' < k is a prefix of the draw with k.  Fewer than k eligible
 * items: the remaining slots are written -1 and *fail_flag is raised.  users[s] outside [0, num_users): the k slots
 * are written 0 and *err_flag is raised.  A CSR row with indptr[u] < 0, indptr[u + 1] < indptr[u] or
 * indptr[u + 1] > nnz is read as empty and raises *err_flag.  Both flags are device int32, nullable.
 * 1 <= k <= CTR_GROUP_MAX_K, 1 <= num_items < 2^31, num_users >= 1, nnz >= 0 (CTR_EINVAL otherwise); n == 0 is a
 * no-op.
 * ctr_group_rank ranks the positive of every group.  scores: n groups of 1 + k float32, slot 0 the positive,
 * leading dimension ld >= 1 + k (ld == 1 + k: the flat prediction vector of an evaluation pass).
 *   rank[g]  = #{ j in 1..k : !(scores[g, j] < scores[g, 0]) }
 *   hist[r] += #{ g : rank[g] == r },  r = 0..k
 * The one comparison makes ties and NaN count against the positive.  ranks_out (n) int32 is nullable; hist (k + 1)
 * int64 is ADDED to (integer atomics: exact, independent of the launch geometry), the caller zeroes it.
 * 1 <= k <= CTR_GROUP_MAX_K (CTR_EINVAL otherwise), n <= 2^40 (CTR_ELIMIT beyond); n == 0 is a no-op.
 * ---------------------------------------------------------------------- */
#define CTR_GROUP_MAX_K 4095
int ctr_eval_candidates(const int64_t* users, const int64_t* items, int64_t n, const int64_t* indptr,
                        const int32_t* indices, int64_t nnz, int64_t num_users, int64_t num_items, int k,
                        uint64_t seed, int64_t* cand, int64_t ld, int32_t* err_flag, int32_t* fail_flag, void* stream);
int ctr_group_rank(const float* scores, int64_t ld, int64_t n, int k, int32_t* ranks_out, int64_t* hist,
                   void* stream);

/* ------------------------------------------------------------------------
 * Score-level evaluation (csrc/score_eval.hip): log-loss, confusion counts, calibration and RMSE in one pass over
 * (prob, target), and the integer counts behind every user's own AUC (GAUC).  prob / target: n contiguous float32.
 * Class rule: a sample is positive iff target > 0.5f (a NaN target is negative); a prediction is hard iff
 * prob >= 0.5f.
 * ctr_score_counts.  counts (8) int64 = {positives, negatives, tp, fp, fn, tn, bad, 0}, bad = #{prob NaN or outside
 * [0, 1]}, ADDED to by integer atomics: the caller zeroes it.  sums: ceil(n / CTR_SCORE_CHUNK) rows of 4 float64, every
 * row STORED; row c, over the samples [c CTR_SCORE_CHUNK, min(n, (c + 1) CTR_SCORE_CHUNK)):
 *   [0] sum of the fp32 term -(y max(logf(p), -100) + (1 - y) max(logf(1.0f - p), -100)), widened to double; the max
 *       is fmaxf, which drops a NaN: a NaN logarithm (p NaN, p < 0, p > 1) counts as -100
 *   [1] sum p      [2] sum ((double) p - (double) y)^2      [3] sum y
 * A row is summed in a fixed order by one workgroup and depends on its chunk's data only; the caller adds the rows in
 * float64 in chunk order, so the totals are bitwise reproducible.  n == 0 is a no-op; n < 0 or a null pointer with
 * n > 0 is CTR_EINVAL.
 * ctr_gauc_groups.  Group g holds the samples order[offsets[g] .. offsets[g + 1]); order (n) int32, offsets
 * (num_groups + 1) int64.  small_groups (num_small) lists the groups of at most CTR_GAUC_SMALL samples; every larger
 * group g of s samples has ceil(s / CTR_GAUC_SLAB) slabs (slab_group = g, slab_first = 0, CTR_GAUC_SLAB, ..).  With i
 * over the positives of group g and j over its negatives:
 *   pos_out[g] = #positives     neg_out[g] = #negatives                                 (int32, stored)
 *   u2_out[g] += sum_i sum_j ( 2 [prob_j < prob_i] + [prob_j == prob_i] )               (int64, ADDED to: zero it)
 * so that AUC_g = u2 / (2 pos neg).  IEEE comparisons: a NaN score on either side adds 0, -0.0 == 0.0.  Integers only:
 * exact, whatever the launch geometry or the order of the atomics.  An order entry outside [0, n) is skipped and raises
 * *err_flag (device int32, nullable); so does a work item that does not fit the plan (group id outside
 * [0, num_groups), offsets outside 0 <= lo <= hi <= n, a small group longer than CTR_GAUC_SMALL, a slab that starts
 * outside its group), which is skipped whole.  n or num_groups >= 2^31 is CTR_ELIMIT; a negative count, or a null
 * pointer with work to do, is CTR_EINVAL; num_groups == 0 is a no-op.
 * ---------------------------------------------------------------------- */
#define CTR_SCORE_CHUNK 65536
#define CTR_GAUC_SMALL 64      /* groups up to this size: one wave each */
#define CTR_GAUC_SLAB  1024    /* larger groups: one work item per this many samples */
int ctr_score_counts(const float* prob, const float* target, int64_t n, int64_t* counts, double* sums, void* stream);
int ctr_gauc_groups(const float* prob, const float* target, int64_t n, const int32_t* order, const int64_t* offsets,
                    int64_t num_groups, const int32_t* small_groups, int64_t num_small, const int32_t* slab_group,
                    const int32_t* slab_first, int64_t num_slabs, int32_t* pos_out, int32_t* neg_out, int64_t* u2_out,
                    int32_t* err_flag, void* stream);

/* ------------------------------------------------------------------------
 * Head folding: a linear layer W (n x k, bias b) whose output feeds ONLY a single-unit layer u is the
 * k-wide dot product  (h W^T + b).u + b2 == h.v + c,  v = W^T u,  c = b.u + b2.  NeuralCF ends like
 * that (model/neuralcf.py:27 linear, :50-56 cat + linear2): folding per step keeps the 8 -> mf_dim
 * layer, its (B, mf_dim) output and that output's gradient out of the batch-sized work.
 *   u_full = [ p columns that pass through (the GMF half of linear2.weight) | n columns fed by W ]
 * fwd: wfold[0:p] = u_full[0:p], wfold[p:p+k] = W^T u, cfold[0] = b.u + b2[0]   (b, b2 may be null)
 * bwd: from gwfold (p+k) = d/d wfold and gc[0] = d/d cfold, all outputs ACCUMULATED (nullable):
 *      gu_full += [gwfold[0:p] | W gwfold[p:] + b gc],  gw += u (x) gwfold[p:],  gb += u gc,  gb2 += gc.
 * ---------------------------------------------------------------------- */
int ctr_fold_head_fwd(const float* u_full, int p, const float* w, int64_t ldw, const float* b, const float* b2, int n,
                      int k, float* wfold, float* cfold, void* stream);
int ctr_fold_head_bwd(const float* u_full, int p, const float* w, int64_t ldw, const float* b, int n, int k,
                      const float* gwfold, const float* gc, float* gu_full, float* gw, int64_t ldgw, float* gb,
                      float* gb2, void* stream);

/* ------------------------------------------------------------------------
 * The rest of a train_loop body (trainer/trainer.py:37-39).
 * ---------------------------------------------------------------------- */

/* torch.nn.BCELoss() with mean reduction (every script, e.g. scripts/pnn.py:54):
 * loss[0] = mean_i -[t_i*max(log p_i,-100) + (1-t_i)*max(log(1-p_i),-100)].
 * prob/target: element i at [i*ld]; workspace: >= 256 floats of device scratch; ticket: one device
 * word that is ZERO on entry and zero again when the call has run (the single launch finds its
 * last workgroup with it) -- allocate it once per stream, zeroed, and keep passing it.
 * gprob_unit (nullable, n contiguous floats): receives what ctr_bce_bwd would write for gloss[0] == 1
 * (bit-identical), so that a caller who knows its upstream gradient is 1 -- loss.backward() -- needs no
 * second launch. */
int ctr_bce_fwd(const float* prob, int64_t ldp, const float* target, int64_t ldt, int64_t n, float* loss,
                float* workspace, int64_t workspace_floats, unsigned int* ticket, float* gprob_unit, void* stream);
/* gprob[i*ldg] = (p_i - t_i) / max(p_i (1-p_i), 1e-12) * gloss[0] / n */
int ctr_bce_bwd(const float* prob, int64_t ldp, const float* target, int64_t ldt, int64_t n,
                const float* gloss, float* gprob, int64_t ldg, void* stream);

/* Ranking losses over groups of 1 positive + k negatives (csrc/group_loss.hip): what a model scored by ctr_group_rank
 * trains on, over the batches of ctr_load_batch_groups.  The models return probabilities, so the losses take
 * probabilities like ctr_bce_fwd.  n groups of 1 + k samples, sample j of group g at prob[(g (1 + k) + j) * ldp],
 * slot 0 the positive:
 *   z_i  = max(log p_i, -100) - max(log(1 - p_i), -100)         (1 - p formed in fp32; a NaN stays a NaN)
 *   kind 0, BPR:      L = 1/(n k) * sum_g sum_{j=1..k} softplus(z_gj - z_g0),  softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   kind 1, softmax:  L = 1/n * sum_g [ m_g + log sum_{j=0..k} exp(z_gj - m_g) - z_g0 ],   m_g = max_j z_gj
 *   dL/dz:    BPR      dz_gj = sigmoid(z_gj - z_g0) / (n k)  (j >= 1),   dz_g0 = -sum_j dz_gj
 *             softmax  dz_gj = (softmax_j - [j == 0]) / n
 *   dL/dp_i = dz_i / max(p_i (1 - p_i), 1e-12) * gloss[0]       (ctr_bce_bwd's floor; composes with the model's
 *                                                                sigmoid backward to exactly dz)
 * ctr_group_loss_fwd writes loss[0] in ONE launch; workspace (>= 256 floats), ticket and gprob_unit (nullable,
 * n (1 + k) contiguous floats: what ctr_group_loss_bwd writes for gloss[0] == 1, bit-identical) are ctr_bce_fwd's, and
 * the ticket word may be the same one.  The loss is bitwise reproducible from run to run.
 * ctr_group_loss_bwd writes gprob[i * ldg] for every sample i.
 * kind outside {0, 1}, k outside [1, CTR_GROUP_MAX_K], n < 1 (a mean over nothing), n > 2^40, a null pointer or a
 * stride below 1 is CTR_EINVAL; fewer workspace floats than workgroups is CTR_ELIMIT. */
int ctr_group_loss_fwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, float* loss, float* workspace,
                       int64_t workspace_floats, unsigned int* ticket, float* gprob_unit, void* stream);
int ctr_group_loss_bwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, const float* gloss, float* gprob,
                       int64_t ldg, void* stream);
/* The logQ-corrected softmax: the two entry points above with z'_i = z_i - logq[i * ldq] in place of z_i for every
 * sample, the positive's included (one fp32 subtraction before the maximum); logq[i * ldq] = log q(item of sample i),
 * what ctr_load_batch_groups_pop writes to logq_out.  Everything else, launches and bitwise reproducibility included,
 * is as above; a null logq is the uncorrected loss, and logq == 0 everywhere gives its bits.  kind 0 with a logq, or a
 * logq with ldq < 1, is CTR_EINVAL.  A NaN in logq is a NaN loss. */
int ctr_group_loss_logq_fwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, float* loss, float* workspace,
                            int64_t workspace_floats, unsigned int* ticket, float* gprob_unit, const float* logq,
                            int64_t ldq, void* stream);
int ctr_group_loss_logq_bwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, const float* gloss, float* gprob,
                            int64_t ldg, const float* logq, int64_t ldq, void* stream);

/* history-position part of the DIN / DIEN table gradient for the E-wide operand (CTR_DIN_H):
 *   gtable[hist[b,l], :] += gh[(b*len+l)*ldgh + 0:E] + attn[b*len+l] * gpool[(summed ? b : b*len+l)*ldgp + 0:E]
 * gh = gradient of the attention MLP's E-wide input, gpool = gradient of the pooled output (model/din.py:47) or of
 * the per-position outputs (model/dien.py:37).  fp32 atomics, row 0 pre-reduced per workgroup.  dim a power of two
 * <= 256.  The target rows are scattered separately (ctr_embed_bwd with the target ids). */
int ctr_din_scatter_bwd(const int64_t* hist, int64_t vocab, int64_t batch, int len, int dim, const float* gh,
                        int64_t ldgh, const float* attn, const float* gpool, int64_t ldgp, int summed, float* gtable,
                        void* stream);

/* FFM forward in one launch (model/ffm.py:46-86): x is the (batch, >= 45) feature matrix; tables[12] the
 * field-aware tables in the order age_user, age_item, gender_user, gender_item, occupation_user, occupation_item,
 * movie_user, movie_item, userid_user, userid_item, itemid_user, itemid_item (each (vocab, dim), dim in
 * {8, 16, 32, 64}; the bag tables have 1 / 2 / 21 / 19 rows, model/ffm.py:11-26); user1 / item1 the (vocab, 1)
 * bias tables, lin_w / lin_b the Linear(43, 1).  Writes emb (batch, 12*dim) -- the vectors, identical to what
 * ctr_embed_fwd produces for the same field list, kept for the backward -- and
 *   prob[b*ldp] = sigmoid(user1[u] + item1[i] + sum_c (x[b, 2+c] + cross) lin_w[c] + lin_b),
 *   cross = the 15 dot products of ffm.py:62-80 summed left to right. */
int ctr_ffm_fused_fwd(const float* x, int64_t ldx, int64_t batch, int dim, const float* const* tables,
                      int64_t num_users, int64_t num_items, const float* user1, const float* item1,
                      const float* lin_w, const float* lin_b, float* emb, int64_t lde, float* prob, int64_t ldp,
                      int32_t* err_flag, void* stream);

/* backward of ctr_ffm_fused_fwd's head and dot products from the emb it wrote: dz = gprob * prob (1 - prob);
 * guser1[u] += dz, gitem1[i] += dz (fp32 atomics), glin_b += sum dz, glin_w[c] += sum dz (x[b,2+c] + cross)
 * (fixed-order partials through the workspace, >= 1024 * 44 floats), and
 * gemb[b, f*dim : (f+1)*dim] = dz * sum(lin_w) * (sum of the vectors paired with f in ffm.py:62-80), which
 * ctr_embed_bwd then turns into the table gradients.  Any gradient pointer may be NULL. */
int ctr_ffm_fused_bwd(const float* x, int64_t ldx, int64_t batch, int dim, const float* emb, int64_t lde,
                      int64_t num_users, int64_t num_items, const float* lin_w, const float* prob, int64_t ldp,
                      const float* gprob, int64_t ldgp, float* guser1, float* gitem1, float* glin_w, float* glin_b,
                      float* gemb, int64_t ldg, float* workspace, int64_t workspace_floats, void* stream);

/* DIN attention on the E-wide operand (model/din.py:39-44: W1 [h, h-t, t] = (Wa+Wb) h + (Wc-Wb) t, so the
 * first attention layer over all B*L positions only contracts the E columns of h; the per-sample term
 * u[b] = (Wc-Wb) t_b + b1 is added per GROUP of L consecutive rows):
 *   y[i, :] = act(x[i, :] W^T + bias + res[i / group, :])       (bias nullable; n <= 128)
 * mask (nullable; n % 32 == 0, ldmask >= n/32 words): bit (j & 31) of mask[i*ldmask + j/32] = (y[i, j] > 0), the
 * ReLU derivative for ctr_linear_dx_masked -- 1 bit instead of a 4-byte re-read of y per element in backward. */
int ctr_linear_group_fwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias /*nullable*/,
                         const float* res, int64_t ldr, int group, float* y, int64_t ldy,
                         uint32_t* mask /*nullable*/, int64_t ldmask, int64_t m, int n, int k, int act, void* stream);
/* input gradient of a layer with the activation mask of the layer BELOW folded into the write-back, plus the
 * per-group column sums the grouped term above needs in backward:
 *   gx[i, :] = ((gy[i, :] * act'(y[i, :])) W) * act_in'(xin[i, :])      (xin = this layer's input = the
 *                                                                         previous layer's activation output)
 *   gsum[i / group, :] += gx[i, :]                                      (nullable; fp32 atomics; group >= 32)
 * xmask (nullable; act_in = RELU, k % 32 == 0): the sign bits ctr_linear_group_fwd wrote for xin, used instead of
 * reading xin.  k <= 128. */
int ctr_linear_dx_masked(const float* w, int64_t ldw, const float* y, int64_t ldy, const float* gy, int64_t ldgy,
                         int act, const float* xin /*nullable with xmask*/, int64_t ldxin, int act_in,
                         const uint32_t* xmask /*nullable*/, int64_t ldxmask, float* gx, int64_t ldgx,
                         float* gsum /*nullable*/, int64_t ldgsum, int group, int64_t m, int n, int k, void* stream);
/* a layer and the single-unit layer on top of it in one pass (DIN attention layers 2 and 3, model/din.py:45-46):
 *   y = act(x W^T + bias)   (m, n) stored as usual,     out[i*ldout] = y[i, :] . u + c[0]     (c nullable)
 * n <= 128: a workgroup holds whole output rows and reduces them in its epilogue. */
int ctr_linear_fwd_dot(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias /*nullable*/,
                       float* y, int64_t ldy, const float* u, const float* c /*nullable*/, float* out, int64_t ldout,
                       int64_t m, int n, int k, int act, void* stream);
/* input gradient of DIN's first attention layer on the E-wide operand, scattered straight into the item table's
 * gradient (model/din.py:35-44 backward: the history rows h = table[hist] receive gX plus the pooling's share):
 *   table[idx[i], :] += gy[i, :] W + attn[i] * gpool[i / group, :]          i < m;  W is (n, k), table (vocab, k)
 * The (m, k) gradient itself is never stored.  fp32 atomics; rows with idx 0 (the padding id, a quarter of DIN's
 * positions) are summed per workgroup first; ids outside [0, vocab) add nothing.  k % 32 == 0, k <= 128,
 * group >= 32, vocab < 2^31. */
int ctr_linear_dx_scatter(const float* w, int64_t ldw, const float* gy, int64_t ldgy, const int64_t* idx,
                          const float* attn, const float* gpool, int64_t ldgp, int group, float* table,
                          int64_t vocab, int64_t m, int n, int k, void* stream);
/* backward of the single-unit score layer y = x w^T + b (model/din.py:46, Linear(.., 1)) with the derivative of
 * the activation that produced x folded in, so the gradient that leaves is already the pre-activation gradient
 * of the layer below:
 *   gx = (gy w) * act_in'(x)   (gx may be x itself -- x is dead after this in DIN's backward)
 *   gw += gy^T x,  gb += sum gy        (either nullable; fixed-order partials through the workspace) */
int ctr_linear_n1_bwd_masked(const float* x, int64_t ldx, const float* w, const float* gy, int64_t ldgy, int act_in,
                             float* gx, int64_t ldgx, float* gw /*nullable*/, float* gb /*nullable*/, int64_t m, int k,
                             float* workspace, int64_t workspace_floats, void* stream);

/* ---- opt-in sparse mode of the embedding gradient / optimizer (replaces, for the rows a
 * batch touches, what `optim.Adam(model.parameters(), lr, weight_decay=1e-5)` does to whole tables:
 * scripts/din.py:87, trainer/trainer.py:39).  A table in sparse mode owns persistent device state: a
 * (vocab, dim) gradient accumulation buffer that is all-zero outside pending rows, one int32 flag per row
 * (0 = clean), an int32 list of pending rows (capacity vocab) with its length, and a ticket word. */
typedef struct ctr_rows_mark_t {
  const void* ids;       /* the ids the backward just scattered: int64, or float32 (ids_are_float) */
  int64_t stride;        /* elements between consecutive ids (a column of a (B,F) matrix: F) */
  int64_t n;             /* number of ids */
  int64_t vocab;         /* rows of the table (< 2^31); ids outside [0, vocab) are skipped */
  int32_t* flags;        /* [vocab] */
  int32_t* rows;         /* [vocab] pending-row list */
  int32_t* count;        /* [1] its length */
  int32_t ids_are_float;
  int32_t reserved;
} ctr_rows_mark_t;

typedef struct ctr_rows_table_t {
  float* param;          /* (vocab, dim); NULL allowed for ctr_rows_discard */
  float* grad;           /* (vocab, dim) persistent accumulation buffer */
  float* exp_avg;
  float* exp_avg_sq;
  int32_t* flags;
  int32_t* rows;
  int32_t* count;
  uint32_t* done;        /* [1] zero-initialised ticket */
  int32_t dim;
  int32_t reserved;
} ctr_rows_table_t;

/* after the scatter kernels have added a batch's gradient rows into `grad`: append every row touched for the
 * first time since the last ctr_adam_rows / ctr_rows_discard to the table's pending list.  One job per
 * (table, id list); several jobs may name the same table.  njobs <= CTR_MAX_FIELDS. */
int ctr_rows_mark(const ctr_rows_mark_t* jobs, int njobs, void* stream);
/* Adam on the pending rows only (same update rule as ctr_adam_step, L2 added to the gradient of those rows),
 * then grad rows, flags and the list are left clean.  `step` = this parameter's 1-based step count. */
int ctr_adam_rows(const ctr_rows_table_t* tables, int ntables, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int64_t step, void* stream);
/* drop the pending gradient rows (what zero_grad means in sparse mode) */
int ctr_rows_discard(const ctr_rows_table_t* tables, int ntables, void* stream);

/* torch.optim.Adam(params, lr, betas, eps, weight_decay) (e.g. scripts/pnn.py:55), one
 * step over all tensors in one launch (16-byte aligned, contiguous fp32):
 *   g += wd*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 *   p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).   tensors: host array. */
#define CTR_ADAM_MAX_TENSORS 64
typedef struct ctr_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} ctr_adam_tensor_t;
int ctr_adam_step(const ctr_adam_tensor_t* tensors, int ntensors, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTRHIP_H */
