/* C ABI of libdcl_tsne.so: exact t-SNE (van der Maaten's tsne.py, the algorithm behind the reference's demo_tsne mode,
 * utils/tsne_visualization.py) of up to a few ten thousand sampled pixel features on gfx950 kernels.
 *
 * A tenth, small library next to the main one, with its own prefix (dts_) and its own binding module (_lib_tsne.py).  The eager
 * composition forms about ten N x N tensors in every one of its iterations; here P [N, N] is the only N x N buffer: the distances
 * of a row live in LDS (or in the row of P itself) while its conditional probabilities are searched, and an iteration reads P
 * once and never writes an N x N quantity.
 *
 * The arithmetic (constants are tsne.py's), all f32:
 *   cond_p      d_j = sum_k (x_ik - x_jk)^2 (difference form, FMA chain over k), shifted by min_{j != i} d_j; beta = 1, bracket
 *               (-inf, inf); H = log sum_j e^{-beta d_j} + beta sum_j d_j e^{-beta d_j} / sum_j e^{-beta d_j}; stop when
 *               |H - log(perplexity)| <= 1e-5 or after 50 tries; H too large: lower = beta, beta doubles while upper is infinite,
 *               else the midpoint; H too small: the mirror image with halving.  P[i, j] = e^{-beta d_j} / sum, P[i, i] = 0.
 *   symmetrize  P <- (P + P^T) / sum(P + P^T), in place, the result bitwise equal to its transpose.
 *   iteration   p = max(4 P, 1e-21) * exaggeration / 4; num = 1 / (1 + |y_i - y_j|^2), num_ii = 0; Z = sum num;
 *               q = max(num / Z, 1e-12); dY_i = sum_j (p - q) num (y_i - y_j); gains += 0.2 where (dY > 0) != (iY > 0), else
 *               gains *= 0.8, then max(gains, 0.01); iY = momentum iY - 500 gains dY; Y += iY; Y -= column means;
 *               KL = sum p log(p / q).
 *
 * Every device entry launches on `stream`, never waits for the device, uses no atomics and no hand-over between the workgroups
 * of a launch (no flags, tickets or spin-waits): sums across workgroups are two-stage, the partials summed in a fixed order at
 * the head of the consuming launch.  Results are bitwise the same from run to run. */
#ifndef DTS_TSNE_H
#define DTS_TSNE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTS_OK 0
#define DTS_EINVAL 1
#define DTS_MAX_D 64        /* feature dimensions at the kernel (after the PCA) */
#define DTS_LDS_ROW 8192    /* a row's distances live in LDS up to this N (32 KiB), above it in the row of P */
#define DTS_SYM_TILE 32     /* symmetrize: a workgroup owns a 32 x 32 tile and its mirror tile */
#define DTS_SYM_GROUPS 1024 /* symmetrize: at most this many workgroups (= partial sums) */
#define DTS_Z_ROWS 256      /* zsum: rows of a workgroup */
#define DTS_Z_COLS 1024     /* zsum: columns of a workgroup */
#define DTS_GRAD_ROWS 8     /* gradient: whole rows of P a workgroup owns */
#define DTS_UPD_ROWS 256    /* update: points of a workgroup */

int dts_version(void);
const char *dts_last_error(void);

/* Host only: 1 when the kernels take X [N, D] at this perplexity: 1 <= D <= DTS_MAX_D, 0 < perplexity < N - 1, N * N < 2^31. */
int dts_supported(int64_t N, int D, double perplexity);

/* ---- the plan: host arithmetic (csrc/dcl_tsne_plan.h), exported for the Python side and its tests ---- */
int dts_plan_row_in_lds(int N);               /* 1: cond_p keeps a row's distances in LDS */
int dts_plan_sym_groups(int N);               /* workgroups of dts_symmetrize = floats of its `part` */
int dts_plan_z_parts(int N);                  /* floats of zpart */
int dts_plan_grad_groups(int N);              /* workgroups of dts_gradient = floats of klpart */
int dts_plan_upd_groups(int N);               /* workgroups of dts_update; colpart holds 2 floats per group */
int dts_plan_grad_vec(uint64_t p_base, int N); /* 1: rows of P are read with 16-byte loads (base on 16 bytes, N % 4 == 0) */
int64_t dts_plan_ws_floats(int N);            /* floats of dts_run's workspace: zpart | klpart | colpart, in this order */
int dts_plan_kl_slots(int n_iter);            /* entries of the KL history: n_iter / 10 */

/* Step 2.  P f32 [N, N] and beta f32 [N] are written; X f32 [N, D].  scratch: 0 = the plan decides where a row's distances live,
 * 1 = in the row of P whatever N is (for tests of that path at small N).  One workgroup per row. */
int dts_cond_p(const float *X, int N, int D, float perplexity, int scratch, float *P, float *beta, void *stream);

/* Step 3, in place.  part: dts_plan_sym_groups(N) floats of workspace (two launches: partial sums, then the update). */
int dts_symmetrize(float *P, int N, float *part, void *stream);

/* zpart[dts_plan_z_parts(N)] = partial sums of num over row blocks x column chunks of Y f32 [N, 2].  Reads Y only. */
int dts_zsum(const float *Y, int N, float *zpart, void *stream);

/* dY f32 [N, 2] from P, Y and the partials of Z (summed at the head of the launch, in a fixed order).  exaggeration: 4 or 1.
 * klpart (or NULL): dts_plan_grad_groups(N) partial sums of p log(p / q), from the same pass over P.  z_out (or NULL): Z. */
int dts_gradient(const float *P, const float *Y, int N, float exaggeration, const float *zpart, float *dY, float *klpart,
                 float *z_out, void *stream);

/* gains, iY and Y [N, 2] updated in place from dY, then Y re-centred (two launches; colpart: 2 * dts_plan_upd_groups(N) floats
 * of workspace).  kl_out (or NULL, then klpart may be NULL): *kl_out = the sum of klpart[dts_plan_grad_groups(N)]. */
int dts_update(const float *dY, float *iY, float *gains, float *Y, int N, float momentum, float *colpart, const float *klpart,
               float *kl_out, void *stream);

/* Iterations [first, last) of step 5, four launches each, no host synchronisation: exaggeration 4 while it <= 100, momentum 0.5
 * while it < 20 else 0.8, and kl_hist[(it + 1) / 10 - 1] = KL when (it + 1) % 10 == 0 (kl_hist: dts_plan_kl_slots(last) floats, or
 * NULL).  dY f32 [N, 2] and ws (dts_plan_ws_floats(N) floats) are workspace. */
int dts_run(const float *P, float *Y, float *iY, float *gains, float *dY, float *ws, int N, int first, int last, float *kl_hist,
            void *stream);

#ifdef __cplusplus
}
#endif
#endif
