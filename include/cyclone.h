/*
 * cyclone.h -- C ABI of libcyclone, the MI355X (gfx950) backend for the MLlib
 * linear-algebra hot path of wmeddie/CycloneML (Spark 3.3 MLlib).
 *
 * Two layers:
 *   - device-pointer entry points (suffix _dev): operands already resident in
 *     HBM, a HIP stream passed as void*.  These are what a multi-GPU driver
 *     (one process per GPU, RCCL all-reduce of the outputs) calls.
 *   - host-pointer entry points over library-owned resident datasets
 *     (cyc_dataset_*): what a JVM shim (JNI / Panama)
 *     binds in place of the per-partition Scala loops.
 *
 * Conventions
 *   - Every function returns CYC_OK (0) or a CYC_ERR_* code; the message is
 *     thread-local and read with cyc_last_error().  CYC_ERR_INVALID_ARG
 *     carries the reference's `require` text (IllegalArgumentException).
 *   - All floating point is IEEE fp64; indices are int32 (Spark's Int) and row
 *     counts int64.  Dense matrices are row-major (InstanceBlock / an RDD of
 *     DenseVector rows); CSR is (rowptr int64[n+1], colidx int32, values).
 *   - Accumulating outputs (sums, gradients, Gramians, loss/weight sums) are
 *     ADDED to, like the reference aggregators' `add`; zero them first.
 *   - There is no CPU fallback: without a gfx950 device every entry point
 *     returns CYC_ERR_NO_DEVICE.
 *   - Calls on one plan/dataset are serialized by the caller (a plan owns
 *     scratch memory); distinct plans may be used from distinct threads.
 */
#ifndef CYCLONE_H
#define CYCLONE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CYC_OK 0
#define CYC_ERR_INVALID_ARG 1 /* a reference `require` failed              */
#define CYC_ERR_HIP 2         /* HIP runtime error                          */
#define CYC_ERR_ALLOC 3       /* device allocation failed                   */
#define CYC_ERR_UNSUPPORTED 4 /* shape outside what the kernels support     */
#define CYC_ERR_NO_DEVICE 5   /* no usable gfx950 device                    */
#define CYC_ERR_ASSERTION 6   /* a reference `assert` failed (AssertionError) */

/* ------------------------------------------------------------------ misc */
const char* cyc_last_error(void);
int cyc_version(void); /* major*10000 + minor*100 + patch */
int cyc_device_count(int* count);
int cyc_set_device(int device);
int cyc_synchronize(void* stream);

/* Measurement hook (bench.py's roofline): while enabled, every launch of a
 * workload's dominant kernel (k_kmeans_assign, k_gram_dma, k_mlr_margins,
 * k_mlr_grad, k_binlog_dense, k_binlog_csr) is bracketed by HIP events on the
 * stream it runs on.  query waits for the recorded events of `kernel`,
 * returns their summed time (ms) and count, and forgets them. */
int cyc_profile_enable(int enable);
int cyc_profile_query(const char* kernel, double* total_ms, int64_t* launches);
/* Restrict the timers to the comma-separated kernel names (NULL or "": all
 * of them), so a timed region carries only the events it reads. */
int cyc_profile_only(const char* kernels);

/* ------------------------------------------------------------- vectors */
/* norms[i] = Vectors.norm(row i, 2.0) bit-exactly (mllib/linalg/Vectors.scala:
 * 489-514, sequential sum of squares, correctly rounded sqrt).              */
int cyc_row_norms_dev(const double* X, int64_t n, int32_t d, double* norms, void* stream);

/* ---------------------------------------------------------------- KMeans */
/* Replaces the Lloyd-iteration body of mllib/clustering/KMeans.scala:275-334:
 * DistanceMeasure.computeStatistics[Distributedly] (DistanceMeasure.scala:
 * 48-118), EuclideanDistanceMeasure.findClosest with statistics (:282-313),
 * updateClusterSum / clusterWeightSum / costAccum (KMeans.scala:299-304) and
 * centroid + isCenterConverged (:322-330).  Dense points and centers.
 *
 * Assignments and per-point costs are bit-identical to the reference's
 * findClosest.  Sums/weights/cost are summed in a fixed (deterministic) order
 * that differs from a Spark partitioning, so they agree to ~1e-15 relative.  */
typedef struct cyc_kmeans_plan_s* cyc_kmeans_plan;

int cyc_kmeans_plan_create(int32_t d, int32_t k, int64_t max_rows, cyc_kmeans_plan* plan);
int cyc_kmeans_plan_destroy(cyc_kmeans_plan plan);

/* The plan's DistanceMeasure (DistanceMeasure.decodeFromString,
 * DistanceMeasure.scala:241-247): CYC_DISTANCE_EUCLIDEAN (the default) or
 * CYC_DISTANCE_COSINE (CosineDistanceMeasure, :395-514).  Set it before any
 * other call on the plan; a row image (cyc_kmeans_rows_create) is built for
 * the plan's measure.  With COSINE every call below uses the cosine forms:
 * distance 1 - dot(c, x) / |c| / |x| (:453-456), the statistic
 * 1 - sqrt(1 - d / 2) (:412-417), updateClusterSum axpy(w / |x|, x, sum)
 * (:466-469), the unit-norm centroid whose norm is set to 1.0 (:477-483) and
 * isCenterConverged distance <= epsilon (:161-166); a zero-length (or NaN)
 * norm returns CYC_ERR_ASSERTION with the reference's assert text.  Dense and
 * CSR points (sparse: dot(sparse, dense) and the sparse axpy). */
#define CYC_DISTANCE_EUCLIDEAN 0
#define CYC_DISTANCE_COSINE 1
int cyc_kmeans_plan_set_distance_measure(cyc_kmeans_plan plan, int32_t measure);

/* computeStatistics for the given centers: fills the plan's packed k(k+1)/2
 * statistics (and copies them to stats_out if non-NULL, device memory).
 * With COSINE the centers' norms are computed here (new VectorWithNorm(c),
 * as KMeansModel's lazy statistics do); cyc_kmeans_accumulate_dev uses the
 * cnorm it is given. */
int cyc_kmeans_stats_dev(cyc_kmeans_plan plan, const double* C, double* stats_out, void* stream);

/* Per-fit row image (KMeans.scala:263-270 caches the rows with their norms
 * once per fit; this caches a second view of the same rows): the int8
 * three-limb fixed-point image that the exact-integer screen streams, 3 bytes
 * per (64-padded) element + 8 bytes per row.  Built once from X (n x d device
 * rows); X must not change while the image is used.  For d > 512 the image is
 * empty and the calls below use the bf16 / fp64 screens instead.  Passing the
 * image is optional everywhere (NULL = no i8 tier).
 * The norms passed with an image (xnorm of cyc_kmeans_accumulate_dev) are
 * fixed for its lifetime, as its rows are: the first accumulate call with a
 * given (xnorm pointer, n) checks the rows' norms for the reference's
 * require(norm >= 0), the image keeps that result, and later calls with the
 * same pointer and n check the centers alone (same message on every call).
 * Norms at another address are checked afresh. */
typedef struct cyc_kmeans_rows_s* cyc_kmeans_rows;
int cyc_kmeans_rows_create(cyc_kmeans_plan plan, const double* X, int64_t n, void* stream,
                           cyc_kmeans_rows* rows);
int cyc_kmeans_rows_destroy(cyc_kmeans_rows rows);
int64_t cyc_kmeans_rows_bytes(cyc_kmeans_rows rows);

/* Carried bounds (Hamerly's, per fit): with a row image, every
 * cyc_kmeans_accumulate_dev call (Euclidean, d <= 256, 96 < k <= 4096)
 * keeps per row an upper bound of its distance to its assigned center and a
 * lower bound to every other center, for the centers of that call.  The next
 * call moves them by each center's drift (triangle inequality) and skips the
 * screen only for rows whose moved bounds still separate the assigned center
 * from every other by more than the reference's rounding slack
 * (2^-29 (|x|^2 + max |c|^2)) -- the pruned reference loop (DistanceMeasure.
 * scala:282-313) returns that same index, so assignments stay bit-identical;
 * every other row is screened as before.  The first call of a fit screens
 * every row.  State of the row image (one fit: one image, one Lloyd loop);
 * cyc_kmeans_assign_dev / point_cost_dev neither use nor change it.
 * set_bounds(rows, 0) turns it off (and either call drops the state; the
 * environment CYC_KMEANS_BOUNDS=0 turns it off for every image).
 * bounds_info: the accumulate calls that used it and the rows they screened
 * (the rest kept their carried assignment); synchronises the device. */
int cyc_kmeans_rows_set_bounds(cyc_kmeans_rows rows, int32_t enable);
int cyc_kmeans_rows_bounds_info(cyc_kmeans_rows rows, int64_t* calls, int64_t* screened_rows);
/* Rows whose bounds failed but whose carried candidate set (the three-limb
 * candidate tier's, with a lower bound for every center outside it) was
 * re-checked instead of a full screen -- certified there or passed on to
 * the screen (and then also counted in screened_rows).  Synchronises. */
int cyc_kmeans_rows_bounds_rechecked(cyc_kmeans_rows rows, int64_t* rechecked_rows);

/* Incremental cluster sums across one fit's cyc_kmeans_accumulate_dev calls
 * on these rows (round 6; on by default, CYC_KMEANS_INCR=0 turns the default
 * off).  Applies with the carried bounds, weights == NULL and cost == NULL
 * (no per-row costs).  The rows object keeps each cluster's sums, count and
 * the sum of squared distances to a reference point.  A call whose moved rows
 * are at most n / 16 updates them by those rows alone.  The cost for the call's
 * centers then comes from Q + 2 (P - c).(S - W P) + W |P - c|^2, with its
 * rounding bounded on the device.  A bound above 2^-40 of the cost, too many
 * moved rows or no prior state run the full pass over every row (which resets
 * the state).  The caller's buffers receive sums, weights and cost either way;
 * the assignments are unaffected.  Replaces nothing in the reference: its
 * KMeans.scala:287-306 re-sums every point.  enable = 0 drops the state. */
int cyc_kmeans_rows_set_incremental(cyc_kmeans_rows rows, int32_t enable);
/* Calls that took the incremental path, and the moved rows they folded, over
 * the object's life.  Synchronises. */
int cyc_kmeans_rows_incremental_info(cyc_kmeans_rows rows, int64_t* incremental_calls,
                                     int64_t* moved_rows);

/* findClosest(centers, stats, point) for n points (stats from the last
 * cyc_kmeans_stats_dev on this plan).  assign[n], cost[n] device outputs.
 * rows: NULL or the image of exactly these X, n.
 * *n_exact_out (host, may be NULL) receives how many points needed the
 * exact-emulation path (ties / near ties the screens cannot separate). */
int cyc_kmeans_assign_dev(cyc_kmeans_plan plan, const double* X, const double* xnorm,
                          cyc_kmeans_rows rows, int64_t n, const double* C, const double* cnorm,
                          int32_t* assign, double* cost, int64_t* n_exact_out, void* stream);

/* findClosest(centers, point) WITHOUT statistics (DistanceMeasure.scala:
 * 318-340): the loop behind DistanceMeasure.pointCost (:152-156), i.e.
 * KMeansModel.computeCost (mllib/clustering/KMeansModel.scala:110-117) and the
 * k-means|| cost updates (KMeans.scala:379-402).  Needs no statistics on the
 * plan.  assign[n] / cost[n] bit-identical to the reference loop (a point no
 * center reaches keeps cost +Infinity, index 0). */
int cyc_kmeans_point_cost_dev(cyc_kmeans_plan plan, const double* X, const double* xnorm,
                              cyc_kmeans_rows rows, int64_t n, const double* C,
                              const double* cnorm, int32_t* assign, double* cost, void* stream);

/* Screening tiers of the last cyc_kmeans_assign_dev call that asked for
 * n_exact_out: rows the first screen (i8 with a row image, else bf16x3) left
 * to the fp64 MFMA screen (all rows when neither runs), and rows left to the
 * exact emulation. */
int cyc_kmeans_last_tiers(cyc_kmeans_plan plan, int64_t* fp64_screen_rows, int64_t* exact_rows);
/* Rows the d <= 256 screen's two-limb i8 pass left to its three-limb pass
 * (rows whose candidate set it could not list) on the last counted assign (-1 when that call ran no two-limb pass).  A
 * statistic of the tiered findClosest; no reference counterpart. */
int cyc_kmeans_last_screen(cyc_kmeans_plan plan, int64_t* three_limb_rows);
/* Rows the two-limb pass handed to its candidate pass (exact fp64 distances
 * to the <= 6 centers its bounds could not exclude) on the last counted
 * assign (-1 when no two-limb pass ran).  Also a tier statistic. */
int cyc_kmeans_last_candidates(cyc_kmeans_plan plan, int64_t* candidate_rows);
/* Of those, the rows the three-limb candidate tier (exact integer limb
 * products over the candidates, k_screen_cands3) could not certify and left
 * to the fp64 candidate pass (-1 when the tier did not run).  A tier
 * statistic; no reference counterpart. */
int cyc_kmeans_last_candidates3(cyc_kmeans_plan plan, int64_t* fp64_rows);
/* The last i8 screen's one-limb pass + two-limb refinement (d <= 256,
 * 96 < k <= 4096): rows the one-limb pass listed with their candidate
 * centers, rows handed to the full two-limb pass, and the candidate centers
 * the refinement screened in total (each wave 32 listed rows); all -1 when
 * that screen ran the two-limb pass over every center.  Statistics of the
 * tiered findClosest; no reference counterpart. */
int cyc_kmeans_last_refine(cyc_kmeans_plan plan, int64_t* listed_rows, int64_t* full_rows,
                           int64_t* union_centers);

/* One partition's contribution to a Lloyd iteration: statistics + assign +
 * per-cluster sums.  sums[k*d] += sum of w*x, wsum[k] += sum of w,
 * cost_sum[0] += sum of w*cost.  weights may be NULL (unit weights).
 * rows: NULL or the image of exactly these X, n.  assign/cost (per-row
 * outputs) may be NULL.  All pointers are device memory.
 * xnorm may be NULL with a Euclidean row image: the image's norms (built
 * with it, in another summation order -- within the screens' margins) serve
 * the screens, and the rows the reference loop itself decides
 * (k_assign_exact) get the reference's Vectors.norm computed there, so the
 * results are the same bits as with the caller's norms (the per-fit norm
 * pass of KMeans.scala:263-270 is then not needed). */
int cyc_kmeans_accumulate_dev(cyc_kmeans_plan plan, const double* X, const double* xnorm,
                              cyc_kmeans_rows rows, const double* weights, int64_t n,
                              const double* C, const double* cnorm, double* sums, double* wsum,
                              double* cost_sum, int32_t* assign, double* cost, void* stream);

/* centroid = scal(1/wsum, sum) and a fresh norm for every cluster with
 * wsum > 0; converged_out (device int32) = 1 iff every such center moved by
 * fastSquaredDistance <= epsilon^2. C and cnorm are updated in place. */
int cyc_kmeans_update_dev(cyc_kmeans_plan plan, double* C, double* cnorm, const double* sums,
                          const double* wsum, double epsilon, int32_t* converged_out,
                          void* stream);

/* ClusteringEvaluator's Silhouette (ml/evaluation/ClusteringEvaluator.scala
 * :106-150 -> ClusteringMetrics.silhouette :48-60): the plan's distance
 * measure selects SquaredEuclideanSilhouette (ClusteringMetrics.scala
 * :254-400) or CosineSilhouette (:403-600).  Replaces the two Spark jobs of
 * computeSilhouetteScore: the aggregateByKey of computeClusterStats and the
 * per-row UDF + overallScore.  Rows X (n x d, plan d) with predictions
 * pred[n] in [0, plan k), weights (nullable = 1.0, each >= 0: the
 * checkNonNegativeWeight require, ml/functions.scala:91), xnorm (nullable:
 * computed) = Vectors.norm(x, 2.0).
 * _stats_dev ADDS this shard's cluster statistics into the device buffer
 * stats[k d + 3 k] = [featureSum (k x d) | squaredNormSum (k) | weightSum
 * (k) | rows (k)] (zero it first; all-reduce it across ranks: the combOp).
 * _score_dev, on the merged stats, ADDS sum_i s_i w_i and sum_i w_i of this
 * shard into partial[2] (device; all-reduce, then the score is
 * partial[0] / partial[1]); fewer than two clusters with rows ->
 * CYC_ERR_ASSERTION "assertion failed: Number of clusters must be greater
 * than one." (:391 / :532). */
int cyc_kmeans_silhouette_stats_dev(cyc_kmeans_plan plan, const double* X, const double* xnorm,
                                    int64_t n, const int32_t* pred, const double* weights,
                                    double* stats, void* stream);
int cyc_kmeans_silhouette_score_dev(cyc_kmeans_plan plan, const double* X, const double* xnorm,
                                    int64_t n, const int32_t* pred, const double* weights,
                                    const double* stats, double* partial, void* stream);

/* Sparse (CSR) points against dense centers: KMeansExample's libsvm input
 * (BASELINE configs[0]).  Distances are MLUtils.fastSquaredDistance's
 * norm-trick branch (MLUtils.scala:533-576: BLAS.dot(sparse, dense), the
 * precision bounds and the Vectors.sqdist(sparse, dense) fallback,
 * Vectors.scala:598-622) and findClosest replays the reference loop, so
 * assignments and costs are bit-identical; the cluster sums use the sparse
 * axpy (mllib BLAS.scala:93-112) with fp64 atomics (order-free to rounding).
 * xnorm = Vectors.norm of the stored values (cyc_row_norms_csr_dev).  The
 * plan's d is numFeatures; plans with d > 1216 serve only these calls. */
int cyc_row_norms_csr_dev(const int64_t* rowptr, const double* vals, int64_t n, double* norms,
                          void* stream);
/* statistics from the last cyc_kmeans_stats_dev on this plan */
int cyc_kmeans_assign_csr_dev(cyc_kmeans_plan plan, const int64_t* rowptr, const int32_t* colidx,
                              const double* vals, const double* xnorm, int64_t n, const double* C,
                              const double* cnorm, int32_t* assign, double* cost, void* stream);
/* findClosest(centers, point) without statistics for CSR rows (pointCost). */
int cyc_kmeans_point_cost_csr_dev(cyc_kmeans_plan plan, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* xnorm,
                                  int64_t n, const double* C, const double* cnorm,
                                  int32_t* assign, double* cost, void* stream);
int cyc_kmeans_accumulate_csr_dev(cyc_kmeans_plan plan, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* xnorm,
                                  const double* weights, int64_t n, const double* C,
                                  const double* cnorm, double* sums, double* wsum,
                                  double* cost_sum, int32_t* assign, double* cost, void* stream);

/* k-means|| initialisation, the executor side of one step (KMeans.scala:
 * 398-404): chosen[i] = 1 iff the partition's XORShiftRandom(seed ^ (step <<
 * 16) ^ index) draws nextDouble() < 2.0 * costs[i] * k / sum_costs, one draw
 * per point in the partition's order -- the same points the reference keeps.
 * part_starts (HOST, num_parts + 1 offsets from 0): the shard's rows split
 * into Spark partitions; partition p has index first_part_index + p.
 * seed: the Int `new XORShiftRandom(this.seed).nextInt()` (:377).  costs and
 * chosen (uint8) are device arrays of part_starts[num_parts] entries. */
int cyc_kmeans_parallel_sample_dev(const double* costs, const int64_t* part_starts,
                                   int32_t num_parts, int32_t first_part_index, int32_t seed,
                                   int32_t step, int32_t k, double sum_costs, uint8_t* chosen,
                                   void* stream);
/* XORShiftRandom.hashSeed (core/.../util/random/XORShiftRandom.scala:60-66):
 * the generator's initial state for a Long seed (host). */
uint64_t cyc_xorshift_hash_seed(int64_t seed);

/* ------------------------------------------------------ RowMatrix Gramian */
/* Replaces the BLAS.spr seqOp of RowMatrix.computeGramianMatrix
 * (mllib/linalg/distributed/RowMatrix.scala:130-161) and of
 * computeDenseVectorCovariance (:163-220).  U is the packed upper triangle
 * (column-major, U[j(j+1)/2 + i], i <= j) of n(n+1)/2 doubles; the call adds
 * sum_r x_r x_r^T over the dense row-major rows (x_r - mean if mean != NULL).
 * fp64 MFMA syrk, deterministic fixed-order split-K reduction. */
typedef struct cyc_gramian_plan_s* cyc_gramian_plan;

int cyc_gramian_plan_create(int32_t ncols, cyc_gramian_plan* plan);
int cyc_gramian_plan_destroy(cyc_gramian_plan plan);
int cyc_gramian_accumulate_dev(cyc_gramian_plan plan, const double* X, int64_t nrows,
                               const double* mean, double* U, void* stream);
/* U += sum_r x_r x_r^T and sums[c] += sum_r X[r][c] in one pass over the rows
 * (the column sums ride the syrk's diagonal tiles; sums are the same values
 * as cyc_col_sums_dev's to rounding, not the same bits): the uncentred
 * covariance form of RowMatrix.computeCovariance (covariance). */
int cyc_gramian_accumulate_sums_dev(cyc_gramian_plan plan, const double* X, int64_t nrows,
                                    double* U, double* sums, void* stream);
/* sums[c] += sum over rows of X[r][c] (fixed order): the mean pre-pass of
 * RowMatrix.computeCovariance (Statistics.colStats, :456). */
int cyc_col_sums_dev(cyc_gramian_plan plan, const double* X, int64_t nrows, double* sums,
                     void* stream);
/* The same pass with sumsq[c] += sum over rows of X[r][c]^2 beside it (sums
 * bit-identical to cyc_col_sums_dev; sumsq may be NULL): the column
 * variances that choose computeCovariance's form (covariance). */
int cyc_col_moments_dev(cyc_gramian_plan plan, const double* X, int64_t nrows, double* sums,
                        double* sumsq, void* stream);
/* RowMatrix.triuToFull (:845-867): G (n x n column-major) from U. */
int cyc_triu_to_full_dev(int32_t n, const double* U, double* G, void* stream);
/* computeDenseVectorCovariance's finish (:203-217): G = full(U) / (m - 1). */
int cyc_covariance_finalize_dev(int32_t n, const double* U, int64_t m, double* G, void* stream);
/* The same two passes over CSR rows (rowptr int64[nrows + 1], any base;
 * colidx int32 validated as SparseVector indices): the sparse spr branch of
 * BLAS.spr (mllib/linalg/BLAS.scala:269-298) -- the rows are densified in
 * ~1 GiB chunks and go through the fp64 MFMA syrk, mean subtracted when
 * given (the dense-covariance path on CSR rows) -- and the column sums. */
int cyc_gramian_accumulate_csr_dev(cyc_gramian_plan plan, const int64_t* rowptr,
                                   const int32_t* colidx, const double* vals, int64_t nrows,
                                   const double* mean, double* U, void* stream);
int cyc_col_sums_csr_dev(cyc_gramian_plan plan, const int64_t* rowptr, const int32_t* colidx,
                         const double* vals, int64_t nrows, double* sums, void* stream);
int cyc_col_moments_csr_dev(cyc_gramian_plan plan, const int64_t* rowptr, const int32_t* colidx,
                            const double* vals, int64_t nrows, double* sums, double* sumsq,
                            void* stream);
/* RowMatrix.isSparseMatrix (:439-441): *count (device int64) = rows whose
 * sparsity() = 1 - numNonzeros / ncols is below 0.5, over dense X OR CSR
 * (rowptr, vals); the matrix is sparse iff the count (summed over ranks) is 0. */
int cyc_rowmatrix_dense_rows_dev(const double* X, const int64_t* rowptr, const double* vals,
                                 int64_t nrows, int32_t ncols, int64_t* count, void* stream);
/* computeSparseVectorCovariance (:222-246) from the packed Gramian U:
 * G(i, j) = U(i, j) / (m - 1) - (m / (m - 1) * mean(i)) * mean(j), i <= j,
 * mirrored (n x n column-major). */
int cyc_sparse_covariance_finalize_dev(int32_t n, const double* U, int64_t m, const double* mean,
                                       double* G, void* stream);
/* RowMatrix.multiply (:400-423), the pass behind computeSVD's U and
 * PCAModel.transform:
 * Y (nrows x k, row-major) = X (nrows x n, row-major) * B (n x k, column-major:
 * Spark's DenseMatrix.values).  All pointers device, fp64.  Y must not overlap
 * X or B.  Any nrows >= 0 (0: no launch), n >= 1, k >= 1, n k <= Int.MaxValue
 * (DenseMatrix's array bound; CYC_ERR_INVALID_ARG otherwise).  Dense rows:
 * fp64 MFMA over 64-column panels of B, one read of X per panel.  CSR rows
 * (rowptr int64[nrows + 1], any base; colidx int32 validated as SparseVector
 * indices): absent entries are skipped, as the reference's sparse dot skips
 * them.  Each Y[i][l] is summed by one wave in a fixed order (no atomics, no
 * split over the contraction): two calls on the same inputs give the same
 * bits, and a NaN or Inf in a row of X or a column of B reaches only the
 * outputs a per-element dot gives it. */
int cyc_rowmatrix_multiply_dev(const double* X, int64_t nrows, int32_t n, const double* B,
                               int32_t k, double* Y, void* stream);
int cyc_rowmatrix_multiply_csr_dev(const int64_t* rowptr, const int32_t* colidx,
                                   const double* vals, int64_t nrows, int32_t n, const double* B,
                                   int32_t k, double* Y, void* stream);

/* ------------------------------------------ WeightedLeastSquares moments */
/* Replaces WeightedLeastSquares.Aggregator.add (ml/optim/
 * WeightedLeastSquares.scala: spr(w, a, aaSum), axpy(w b, a, abSum),
 * axpy(w, a, aSum), bSum, bbSum, wSum), the seqOp of the normal-equation
 * LinearRegression fit.  For the augmented row z = [a, b, 1.0] of width
 * q = numFeatures + 2 the call adds sum_r w_r z_r z_r^T to U, the packed
 * upper triangle (column-major, U[j(j+1)/2 + i], i <= j) of q(q+1)/2
 * doubles: aaSum is its leading block, abSum column numFeatures, bbSum entry
 * (numFeatures, numFeatures), aSum column numFeatures + 1, bSum entry
 * (numFeatures, numFeatures + 1) and wSum the last entry.  Moments of
 * several calls (or ranks) merge by addition.  w may be NULL (all weights
 * 1).  Rows of weight 0 contribute nothing, whatever their features hold.
 * A negative or NaN weight fails the call with "requirement failed: Negative
 * weight ..." (the call synchronizes the stream to read the flag).
 * numFeatures > 4096 (WeightedLeastSquares.MAX_NUM_FEATURES) fails at plan
 * creation with the reference's message.  fp64 MFMA syrk, deterministic
 * fixed-order split-K reduction. */
typedef struct cyc_wls_plan_s* cyc_wls_plan;

int cyc_wls_plan_create(int32_t numFeatures, cyc_wls_plan* plan);
int cyc_wls_plan_destroy(cyc_wls_plan plan);
int cyc_wls_accumulate_dev(cyc_wls_plan plan, const double* X, int64_t nrows, const double* y,
                           const double* w, double* U, void* stream);
/* The same over CSR rows (densified in ~1 GiB chunks, as
 * cyc_gramian_accumulate_csr_dev). */
int cyc_wls_accumulate_csr_dev(cyc_wls_plan plan, const int64_t* rowptr, const int32_t* colidx,
                               const double* vals, int64_t nrows, const double* y,
                               const double* w, double* U, void* stream);
/* Row splits (split-K slabs) of the plan's last syrk launch. */
int cyc_wls_last_splits(cyc_wls_plan plan, int64_t* splits);

/* ------------------------------------- GeneralizedLinearRegression (IRLS) */
/* The per-row passes of ml/regression/GeneralizedLinearRegression.scala
 * around the WLS aggregate above: FamilyAndLink.initialize / reweightFunc
 * (the instances of one IterativelyReweightedLeastSquares iteration), the
 * fitted mean, and the training summary's reductions.  family and link are
 * the codes below; CYC_GLM_TWEEDIE takes CYC_GLM_POWER with linkPower, and
 * variancePower 0 / 1 / 2 is gaussian / poisson / gamma, linkPower 0 / 1 /
 * -1 / 0.5 is log / identity / inverse / sqrt (Family.fromParams,
 * Link.fromParams).  Plan creation fails on a pair the reference rejects, on
 * variancePower in (0, 1) or negative, and on numFeatures outside 1..4096.
 * Rows are dense row-major X (nrows x numFeatures) or CSR; y, w (NULL: 1)
 * and offset (NULL: 0) are device vectors of nrows doubles, coef a device
 * vector of numFeatures doubles.  eta = dot(x, coef) + intercept + offset;
 * with coef == NULL no features are read (X or the CSR arrays may be NULL)
 * and eta = intercept + offset. */
enum {
  CYC_GLM_GAUSSIAN = 0,
  CYC_GLM_BINOMIAL = 1,
  CYC_GLM_POISSON = 2,
  CYC_GLM_GAMMA = 3,
  CYC_GLM_TWEEDIE = 4
};
enum {
  CYC_GLM_IDENTITY = 0,
  CYC_GLM_LOG = 1,
  CYC_GLM_INVERSE = 2,
  CYC_GLM_LOGIT = 3,
  CYC_GLM_PROBIT = 4,
  CYC_GLM_CLOGLOG = 5,
  CYC_GLM_SQRT = 6,
  CYC_GLM_POWER = 7
};
typedef struct cyc_glm_plan_s* cyc_glm_plan;

int cyc_glm_plan_create(int32_t family, int32_t link, double variancePower, double linkPower,
                        int32_t numFeatures, cyc_glm_plan* plan);
int cyc_glm_plan_destroy(cyc_glm_plan plan);
/* One row -> (z, wOut), the label and weight of the next WLS fit.
 * init != 0 (FamilyAndLink.initialize; coef and the features are not read):
 *   mu = family.initialize(y, w), z = link(mu) - offset, wOut = w.
 * init == 0 (reweightFunc): mu = project(unlink(eta)), g = link.deriv(mu),
 *   z = eta - offset + (y - mu) g, wOut = w / (g g V(mu)); a row of weight 0
 *   gives z = 0, wOut = 0 and its features are not read.
 * A label outside the family's domain fails the call with "requirement
 * failed: ..." (the call synchronizes the stream to read the flag). */
int cyc_glm_reweight_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* y,
                         const double* w, const double* offset, const double* coef,
                         double intercept, int32_t init, double* z, double* wOut, void* stream);
int cyc_glm_reweight_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                             const double* vals, int64_t nrows, const double* y, const double* w,
                             const double* offset, const double* coef, double intercept,
                             int32_t init, double* z, double* wOut, void* stream);
/* out[r] = project(unlink(eta_r)) (predict), or eta_r with linkPrediction. */
int cyc_glm_mean_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* offset,
                     const double* coef, double intercept, int32_t linkPrediction, double* out,
                     void* stream);
int cyc_glm_mean_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                         const double* vals, int64_t nrows, const double* offset,
                         const double* coef, double intercept, int32_t linkPrediction,
                         double* out, void* stream);
/* sums (6 device doubles, overwritten) = { sum w, sum w y, the deviance,
 * Pearson's sum w (y - mu)^2 / V(mu), the log-likelihood behind family.aic
 * (gamma: at `dispersion`; 0 for gaussian and tweedie), sum log w } with
 * mu = project(unlink(eta)) (project != 0) or unlink(eta) (the null
 * deviance).  A row of weight 0 adds only its log w and its features are
 * not read.  Per-wave partials folded in a fixed order: two calls on the
 * same input give the same bits. */
int cyc_glm_stats_dev(cyc_glm_plan plan, const double* X, int64_t nrows, const double* y,
                      const double* w, const double* offset, const double* coef,
                      double intercept, int32_t project, double dispersion, double* sums,
                      void* stream);
int cyc_glm_stats_csr_dev(cyc_glm_plan plan, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, int64_t nrows, const double* y, const double* w,
                          const double* offset, const double* coef, double intercept,
                          int32_t project, double dispersion, double* sums, void* stream);

/* ------------------------------------------- linear models: evaluate pass */
/* One read of a shard's rows (dense row-major nrows x numFeatures, or CSR)
 * for a fitted linear model: p_r = x_r . coef + intercept.
 * predict: out[r] = p_r for every row.
 * stats: with e_r = y_r - p_r, out (10 device doubles, overwritten) =
 *   { sum w, sum w y, sum w y^2, sum w (y - center)^2, sum w e, sum w e^2,
 *     sum w |e|, sum w (p - center)^2, min sqrt(w) e, max sqrt(w) e },
 * the extrema over the rows with w > 0 (+inf, -inf if there is none); w may
 * be NULL (all 1).  pred, if not NULL, receives every row's p_r in the same
 * pass.  A row of weight 0 adds to no output.  With pred == NULL its features
 * are not read; with pred they are read for pred[r] alone, so a NaN there
 * reaches that one element and nothing else.  Per-wave partials folded in a
 * fixed order, no floating-point atomics: two calls on the same input give
 * the same bits. */
int cyc_linreg_predict_dev(const double* X, int64_t nrows, int32_t numFeatures,
                           const double* coef, double intercept, double* out, void* stream);
int cyc_linreg_predict_csr_dev(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                               int64_t nrows, int32_t numFeatures, const double* coef,
                               double intercept, double* out, void* stream);
int cyc_linreg_stats_dev(const double* X, int64_t nrows, int32_t numFeatures, const double* y,
                         const double* w, const double* coef, double intercept, double center,
                         double* out, double* pred, void* stream);
int cyc_linreg_stats_csr_dev(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                             int64_t nrows, int32_t numFeatures, const double* y,
                             const double* w, const double* coef, double intercept,
                             double center, double* out, double* pred, void* stream);

/* ---------------------------------------------- logistic block aggregators */
/* BinaryLogisticBlockAggregator.add (ml/optim/aggregator/
 * BinaryLogisticBlockAggregator.scala:81-145) and
 * MultinomialLogisticBlockAggregator.add (...Multinomial...scala:101-189)
 * over every block of a device-resident shard (blocks concatenated: dense
 * row-major n x F, or CSR).  Features are already scaled by inverseStd, as
 * in the reference.  Accumulates into grad (same layout as the coefficients:
 * binary F [+1]; multinomial C x F column-major [+ C intercepts]), *lossSum
 * and *weightSum (device doubles), like the aggregator's add + merge.
 * weights may be NULL (all-unit weights, InstanceBlock's empty array). */
typedef struct cyc_logistic_plan_s* cyc_logistic_plan;

/* Column-major copy of a resident CSR shard, built once (outside the
 * training loop, like InstanceBlock.blokifyWithMaxMemUsage,
 * ml/feature/Instance.scala:146-187) by a stable sort of the nonzeros by
 * (row block, column).  Passing it to cyc_binary_logistic_add_csr_dev
 * replaces the gradient's fp64-atomic scatter by per-column sums
 * (deterministic: blocks in order, each block's rows in order).  Costs 12
 * bytes per nonzero + 8 bytes per (row block, column).
 * rowptr must be zero-based: rowptr[0] == 0 and rowptr[n] == nnz, colidx and
 * vals holding exactly the n rows.  A slice of a larger CSR whose rowptr
 * starts above 0 is refused with CYC_ERR_INVALID_ARG (rebase it first); the
 * SparseVector index checks run before that and name the lowest bad row. */
typedef struct cyc_csc_s* cyc_csc;
int cyc_csc_build_dev(const int64_t* rowptr, const int32_t* colidx, const double* vals,
                      int64_t n, int32_t numFeatures, void* stream, cyc_csc* out);
int cyc_csc_destroy(cyc_csc csc);
int64_t cyc_csc_rows(cyc_csc csc);
int32_t cyc_csc_features(cyc_csc csc);
/* The copy is row-blocked (rows_per_block rows per block): colptr has
 * nblocks * numFeatures + 1 entries, block b / column c spanning
 * [colptr[b F + c], colptr[b F + c + 1]) of rowidx / values. */
int cyc_csc_blocks(cyc_csc csc, int64_t* rows_per_block, int64_t* nblocks);
int cyc_csc_arrays(cyc_csc csc, const int64_t** colptr, const int32_t** rowidx,
                   const double** values);

/* Row-block x column-tile layout of a CSR shard (tiles.hip) for the binary
 * aggregators' two sparse gemv (BinaryLogisticBlockAggregator.scala:97,130;
 * ml/linalg/BLAS.scala:764-805): row blocks of cyc_tiles_row_block() = 2048
 * rows, column chunks of <= 2048 columns; each (row block, chunk) segment
 * holds its nonzeros in CSR order as fp64 values + ids, so both gathers run
 * from LDS.  Two entry formats: CYC_TILES_WIDE, 12 bytes per nonzero (32-bit
 * packed row / column ids); CYC_TILES_COMPACT, 10 bytes per entry (16-bit:
 * the column and the row's step from the segment's previous entry; a step of
 * 31 rows or more takes filler entries).  CYC_TILES_AUTO (the default) lets
 * the first append that holds nonzeros choose: compact when its fillers are
 * at most 1/32 of its nonzeros (dense-enough segments, e.g. config 5's 268
 * nonzeros per segment: 1.3 % fillers), wide otherwise; cyc_tiles_set_format
 * fixes one before the first append.  Built by appending CSR rows
 * (rowptr[rows+1] of any base, colidx sorted within a row as in
 * SparseVector, values) in order: every append except the last holds a
 * whole number of row blocks.  Indices are validated with SparseVector's
 * require messages (ml/linalg/Vectors.scala:617-625).  The CSR input is not
 * referenced afterwards (free it: the layout is the shard's only copy).
 * capacity_*: upper bounds for the whole shard; a compact layout reserves a
 * 6.25 % allowance of filler entries on top. */
typedef struct cyc_tiles_s* cyc_tiles;
enum { CYC_TILES_AUTO = 0, CYC_TILES_WIDE = 1, CYC_TILES_COMPACT = 2 };
int cyc_tiles_create(int32_t numFeatures, int64_t capacity_rows, int64_t capacity_nnz,
                     cyc_tiles* out);
int cyc_tiles_set_format(cyc_tiles tiles, int32_t format);
/* the entry format in use (CYC_TILES_AUTO until decided) */
int32_t cyc_tiles_format(cyc_tiles tiles);
int cyc_tiles_append_dev(cyc_tiles tiles, const int64_t* rowptr, const int32_t* colidx,
                         const double* vals, int64_t rows, void* stream);
int cyc_tiles_destroy(cyc_tiles tiles);
int64_t cyc_tiles_rows(cyc_tiles tiles);
int64_t cyc_tiles_nnz(cyc_tiles tiles);
/* entry positions used (= nnz for the wide format; + fillers for compact) */
int64_t cyc_tiles_entries(cyc_tiles tiles);
int32_t cyc_tiles_features(cyc_tiles tiles);
int64_t cyc_tiles_bytes(cyc_tiles tiles);
int32_t cyc_tiles_row_block(void);
/* add() of the plan's binary aggregator over every row of the layout
 * (BinaryLogisticBlockAggregator.scala:81-145, or the Hinge / LeastSquares /
 * Huber / AFT plans' epilogues): labels / weights (AFT: censors; NULL =
 * unit) have cyc_tiles_rows() entries; inverseStd is required by least
 * squares plans (effectiveCoef) and ignored otherwise.  Two passes over the
 * layout (margins, then gradient), deterministic. */
int cyc_binary_add_tiles_dev(cyc_logistic_plan plan, cyc_tiles tiles, const double* labels,
                             const double* weights, const double* coef, const double* inverseStd,
                             const double* scaledMean, double* grad, double* lossSum,
                             double* weightSum, void* stream);

/* HingeBlockAggregator (ml/optim/aggregator/HingeBlockAggregator.scala:
 * 81-141, LinearSVC's loss): the binary kernels with the hinge epilogue
 * (labels {0,1} -> {-1,1}; loss (1 - y' m) w and multiplier -y' w where the
 * loss is positive).  The aggregator centers whenever it fits an intercept
 * (marginOffset, :62-71), so the plan takes fitIntercept only.  Same
 * arguments, layouts and tolerance as the binary logistic entry points. */
int cyc_hinge_plan_create(int32_t numFeatures, int fitIntercept, cyc_logistic_plan* plan);
int cyc_hinge_add_dense_dev(cyc_logistic_plan plan, const double* X, const double* labels,
                            const double* weights, int64_t n, const double* coef,
                            const double* scaledMean, double* grad, double* lossSum,
                            double* weightSum, void* stream);
int cyc_hinge_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, const double* labels, const double* weights,
                          int64_t n, const double* coef, const double* scaledMean, double* grad,
                          double* lossSum, double* weightSum, cyc_csc csc, void* stream);

/* HuberBlockAggregator (ml/optim/aggregator/HuberBlockAggregator.scala:
 * 41-141, LinearRegression with loss "huber"): the binary kernels with the
 * Huber epilogue.  coef/grad hold F linear terms, the intercept if
 * fitIntercept, then sigma (dim - 1); the aggregator centers whenever it fits
 * an intercept.  epsilon > 1 (LinearRegression's param check). */
int cyc_huber_plan_create(int32_t numFeatures, int fitIntercept, double epsilon,
                          cyc_logistic_plan* plan);
int cyc_huber_add_dense_dev(cyc_logistic_plan plan, const double* X, const double* labels,
                            const double* weights, int64_t n, const double* coef,
                            const double* scaledMean, double* grad, double* lossSum,
                            double* weightSum, void* stream);
int cyc_huber_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr, const int32_t* colidx,
                          const double* vals, const double* labels, const double* weights,
                          int64_t n, const double* coef, const double* scaledMean, double* grad,
                          double* lossSum, double* weightSum, cyc_csc csc, void* stream);

/* AFTBlockAggregator (ml/optim/aggregator/AFTBlockAggregator.scala:30-130,
 * AFTSurvivalRegression): the binary kernels with the log-linear survival
 * epilogue.  coef/grad: F linear terms, intercept slot, log(sigma) (dim =
 * F + 2; the intercept gradient stays 0 without fitIntercept).  censors[n]
 * (the reference keeps them in Instance.weight) may be NULL (all 1);
 * labels must be > 0 (checked by the caller, as the reference's require);
 * weightSum counts rows. */
int cyc_aft_plan_create(int32_t numFeatures, int fitIntercept, cyc_logistic_plan* plan);
int cyc_aft_add_dense_dev(cyc_logistic_plan plan, const double* X, const double* labels,
                          const double* censors, int64_t n, const double* coef,
                          const double* scaledMean, double* grad, double* lossSum,
                          double* weightSum, void* stream);
int cyc_aft_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr, const int32_t* colidx,
                        const double* vals, const double* labels, const double* censors,
                        int64_t n, const double* coef, const double* scaledMean, double* grad,
                        double* lossSum, double* weightSum, cyc_csc csc, void* stream);

/* LeastSquaresBlockAggregator (ml/optim/aggregator/LeastSquaresBlockAggregator.
 * scala:31-101, LinearRegression's "l-bfgs" loss): the binary kernels with
 * margin (offset or 0) - label/labelStd + x.effectiveCoef, loss w d^2/2 and
 * multiplier w d for every row.  dim = numFeatures (no intercept entry in
 * coef or grad).  coef: the F original coefficients; inverseStd (device, F)
 * zeroes the effective coefficients of constant features (:48-55); the
 * offset labelMean/labelStd - coef.scaledMean (:57-62) uses coef itself.
 * labelStd must be > 0 (the reference's require message). */
int cyc_least_squares_plan_create(int32_t numFeatures, int fitIntercept, double labelStd,
                                  double labelMean, cyc_logistic_plan* plan);
int cyc_least_squares_add_dense_dev(cyc_logistic_plan plan, const double* X,
                                    const double* labels, const double* weights, int64_t n,
                                    const double* coef, const double* inverseStd,
                                    const double* scaledMean, double* grad, double* lossSum,
                                    double* weightSum, void* stream);
int cyc_least_squares_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr,
                                  const int32_t* colidx, const double* vals, const double* labels,
                                  const double* weights, int64_t n, const double* coef,
                                  const double* inverseStd, const double* scaledMean,
                                  double* grad, double* lossSum, double* weightSum, cyc_csc csc,
                                  void* stream);

int cyc_logistic_plan_create(int32_t numFeatures, int32_t numClasses, int fitIntercept,
                             int fitWithMean, cyc_logistic_plan* plan);
int cyc_logistic_plan_destroy(cyc_logistic_plan plan);
int cyc_binary_logistic_add_dense_dev(cyc_logistic_plan plan, const double* X,
                                      const double* labels, const double* weights, int64_t n,
                                      const double* coef, const double* scaledMean, double* grad,
                                      double* lossSum, double* weightSum, void* stream);
int cyc_binary_logistic_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr,
                                    const int32_t* colidx, const double* vals,
                                    const double* labels, const double* weights, int64_t n,
                                    const double* coef, const double* scaledMean, double* grad,
                                    double* lossSum, double* weightSum, cyc_csc csc,
                                    void* stream);
int cyc_multinomial_logistic_add_dense_dev(cyc_logistic_plan plan, const double* X,
                                           const double* labels, const double* weights,
                                           int64_t n, const double* coef,
                                           const double* scaledMean, double* grad,
                                           double* lossSum, double* weightSum, void* stream);
/* CSR rows (the sparse InstanceBlock branch of :122 and :156-162): margins
 * by a wave per row, gradient over the CSC copy (required: built from these
 * rows by cyc_csc_build_dev), numClasses <= 1024. */
int cyc_multinomial_logistic_add_csr_dev(cyc_logistic_plan plan, const int64_t* rowptr,
                                         const int32_t* colidx, const double* vals,
                                         const double* labels, const double* weights, int64_t n,
                                         const double* coef, const double* scaledMean,
                                         double* grad, double* lossSum, double* weightSum,
                                         cyc_csc csc, void* stream);
/* out[i] = the exponential the dense multinomial margins kernel applies to
 * the softmax terms m - max (Utils.softmax's math.exp, ml/impl/Utils.scala:
 * 127-129): e^x for x <= 0 within a few ulp of libm down to -708.4;
 * subnormal results in (-746, -708.4] (about 1e-13 relative error there);
 * 0 below -746 and at -inf; NaN kept (inputs above 0 are outside its
 * contract).  Exported so its accuracy is
 * testable against the host libm. */
int cyc_softmax_exp_dev(const double* x, int64_t n, double* out, void* stream);

/* ---------------------------------------- MultilayerPerceptronClassifier */
/* The feed-forward network of ml/ann/Layer.scala (FeedForwardTopology
 * .multiLayerPerceptron with softmaxOnTop): layers = [n_0 .. n_L], L =
 * nlayers - 1 >= 1, every n_l in 1..4096; affine layers, a sigmoid after
 * each but the last, softmax with cross-entropy on top.  The weights are one
 * flat fp64 device array of sum n_l (n_{l-1} + 1) doubles: for l = 1..L, W_l
 * (column-major n_l x n_{l-1}, W_l[o, i] at i n_l + o), then b_l.  X is
 * dense row-major nrows x n_0, labels fp64 class indices.
 *
 * Rows are evaluated in chunks of chunkRows (0: as many as keep the plan's
 * workspace of 2 chunkRows sum n_l doubles under 1 GiB); the plan owns the
 * workspace and keeps it between calls.
 *
 * cyc_mlp_loss_grad_dev ADDS one shard's share of the DataStacker objective:
 * the shard's rows are cut into blocks of blockSize (the last may be
 * shorter), row i of block b (S_b rows) weighs s_i = 1 / (S_b totalBlocks),
 * totalBlocks = the blocks of all shards; *loss += sum s_i (-log p_i[y_i]),
 * grad (the weights' layout) += sum s_i dl_i/dw.  Only the target class's
 * term of the cross-entropy is taken (the reference's sum over all classes
 * gives NaN once a non-target probability underflows).  A label that is not
 * an integer in [0, n_L) fails the call (CYC_ERR_INVALID_ARG; the call
 * synchronizes the stream to read the flag, and grad / loss are then
 * undefined).  No atomics: two calls on the same inputs add the same bits.
 *
 * cyc_mlp_forward_dev: raw (nrows x n_L, z_L), prob (softmax of z_L), pred
 * (nrows; the argmax of prob as fp64, the lowest index on ties); any of the
 * three may be NULL, not all. */
typedef struct cyc_mlp_plan_s* cyc_mlp_plan;

int cyc_mlp_plan_create(const int32_t* layers, int nlayers, int blockSize, int64_t chunkRows,
                        cyc_mlp_plan* plan);
int cyc_mlp_plan_destroy(cyc_mlp_plan plan);
int cyc_mlp_loss_grad_dev(cyc_mlp_plan plan, const double* X, const double* labels, int64_t nrows,
                          const double* weights, int64_t totalBlocks, double* grad, double* loss,
                          void* stream);
int cyc_mlp_forward_dev(cyc_mlp_plan plan, const double* X, int64_t nrows, const double* weights,
                        double* raw, double* prob, double* pred, void* stream);

/* ------------------------------------------------------- GaussianMixture */
/* The E step and the sufficient statistics of ml/clustering/
 * GaussianMixture.scala (ExpectationAggregator.add) over dense row-major
 * fp64 rows (nrows x numFeatures), 1 <= numFeatures <= 1024, k >= 1.
 *
 * Model (cyc_gmm_set_model_dev, all device fp64): weights (k), means (k x
 * numFeatures, row-major), rootSigmaInv (k matrices numFeatures x
 * numFeatures, row-major: A_j[c, f] at (j d + c) d + f) and u (k) with u_j =
 * -0.5 (d log 2 pi + logPseudoDet_j), the constants of ml/stat/distribution/
 * MultivariateGaussian.scala.  logpdf_j(x) = u_j - 0.5 |A_j (x - mu_j)|^2; the
 * mean is subtracted before the product.  The plan keeps its own copy.
 *
 * Per row i of weight w_i (NULL: all 1): p_ij = EPSILON + weights_j
 * exp(logpdf_j(x_i)), s_i = sum_j p_ij, r_ij = w_i p_ij / s_i, EPSILON =
 * 2^-52.  sums is 1 + k + k d + k d(d+1)/2 doubles, [ll | W | M | S]: ll =
 * sum_i w_i log s_i, W_j = sum_i r_ij, M_j (d) = sum_i r_ij x_i, S_j the
 * packed upper triangle (column-major, S_j[b(b+1)/2 + a], a <= b) of sum_i
 * r_ij x_i x_i^T.  cyc_gmm_accumulate_dev ADDS the rows' share; buffers of
 * several calls (or ranks) merge by addition.  Rows of weight 0 contribute
 * nothing, whatever their features hold.  A negative or NaN weight fails the
 * call with "requirement failed: illegal weight value ..." (the call
 * synchronizes the stream to read the flag; sums is then undefined).
 *
 * cyc_gmm_mstep_dev ADDS W, M and S alone from caller-supplied
 * responsibilities R (nrows x k, row-major); sums[0] is not touched.
 *
 * cyc_gmm_predict_dev: prob (nrows x k, p_ij / s_i at unit row weight),
 * label (nrows int32, the argmax of prob, the lowest index on ties), logpdf
 * (nrows x k, logpdf_j(x_i)); any of the three may be NULL, not all.
 *
 * Rows go through in chunks of chunkRows (0: as many as keep the plan's r
 * workspace of chunkRows k doubles under 1 GiB).  fp64 MFMA, fixed-order
 * reductions, no atomics on doubles: two calls on the same inputs give the
 * same bits. */
typedef struct cyc_gmm_plan_s* cyc_gmm_plan;

int cyc_gmm_plan_create(int32_t k, int32_t numFeatures, int64_t chunkRows, cyc_gmm_plan* plan);
int cyc_gmm_plan_destroy(cyc_gmm_plan plan);
int cyc_gmm_set_model_dev(cyc_gmm_plan plan, const double* weights, const double* means,
                          const double* rootSigmaInv, const double* u, void* stream);
int cyc_gmm_accumulate_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, const double* w,
                           double* sums, void* stream);
int cyc_gmm_mstep_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, const double* R,
                      double* sums, void* stream);
int cyc_gmm_predict_dev(cyc_gmm_plan plan, const double* X, int64_t nrows, double* prob,
                        int32_t* label, double* logpdf, void* stream);

/* ----------------------------------------------------------- NaiveBayes
 * ml/classification/NaiveBayes.scala over row-major fp64 rows (nrows x
 * numFeatures), 1 <= numClasses <= 1024, numFeatures <= 16,776,959.  modelType: 0
 * multinomial, 1 complement, 2 bernoulli, 3 gaussian.
 *
 * Aggregate.  sums is numClasses (1 + numFeatures) doubles (gaussian:
 * numClasses (1 + 2 numFeatures)), [W | S | Q]: W_c = sum of w_i, S_c[j] =
 * sum of w_i x_ij, Q_c[j] = sum of w_i (x_ij x_ij) over the rows of label c
 * (y, nrows doubles; w, nrows doubles or NULL for 1).  The calls ADD the
 * rows' share; buffers of several calls (or ranks) merge by addition.  The
 * same pass checks the rows: label integer-valued in [0, numClasses) (rule
 * 1), weight >= 0 and not NaN (rule 2), values >= 0 (multinomial, complement)
 * or 0 / 1 (bernoulli) (rule 3).  The lowest offending row and its rule go to
 * *badRow / *badRule (-1 / 0 when none; either may be NULL) and the call
 * fails with the reference's message (sums is then undefined).  A bad label
 * is never used as an index.  The call synchronizes the stream to read the
 * flag.  Dense rows only: there is no CSR aggregate.
 *
 * The model comes from the merged sums in closed form on the host
 * (cycloneml_amd/naive_bayes.py m_step).  Scoring on the device is the
 * cyc_nbmodel_* object below.
 *
 * workspaceBytes (0: 256 MiB) bounds the device workspace: the aggregate's
 * run partials (more launches when it is smaller, never other sums).  It
 * grows to one run when smaller than that.  cyc_nb_col_tile (columns of the
 * numFeatures + 1 per lane group of the aggregate), cyc_nb_rows_per_run and
 * cyc_nb_classes_per_pass report the plan's tiling.
 * fp64 throughout, fixed-order reductions, no atomics on doubles: two calls
 * on the same inputs give the same bits. */
typedef struct cyc_nb_plan_s* cyc_nb_plan;

int cyc_nb_plan_create(int32_t numClasses, int32_t numFeatures, int32_t modelType,
                       int64_t workspaceBytes, cyc_nb_plan* plan);
int cyc_nb_plan_destroy(cyc_nb_plan plan);
int64_t cyc_nb_col_tile(cyc_nb_plan plan);
int64_t cyc_nb_rows_per_run(cyc_nb_plan plan);
int64_t cyc_nb_classes_per_pass(cyc_nb_plan plan);
int cyc_nb_aggregate_dev(cyc_nb_plan plan, const double* X, int64_t nrows, const double* y,
                         const double* w, double* sums, int64_t* badRow, int32_t* badRule,
                         void* stream);

/* NaiveBayesModel's predictions over row-major fp64 rows (nrows x
 * numFeatures), numClasses and modelType as above.
 *
 * Operands (device fp64; cycloneml_amd/naive_bayes.py score_operands makes
 * them on the host, so no log, log1p or exp of the model runs on the device):
 * b (numClasses), M (numClasses x numFeatures, row-major) and, gaussian only
 * (else NULL), V (the variances, M's shape) and ls (numClasses, sum_j log
 * V_cj).  cyc_nbmodel_create copies or packs what it needs and synchronizes
 * the stream; the caller's arrays are free afterwards.
 *   multinomial  raw_c = b_c + sum_j x_j M_cj             (b = pi, M = theta)
 *   complement   t_c = sum_j x_j M_cj (b = 0, M = theta), raw_c = t_c - (max_c
 *                t + log sum_c exp(t_c - max))
 *   bernoulli    raw_c = b_c + sum_j x_j M_cj   (b = pi + sum_j L_cj, M = theta
 *                - L, L = log1p(-exp theta))
 *   gaussian     raw_c = b_c - (sum_j (x_j - M_cj)^2 / V_cj + ls_c) / 2
 * In the three linear forms a term with x_j == 0 is skipped (the reference's
 * sparse dot): 0 times a -inf of M adds nothing, a nonzero x_j gives -inf.
 *
 * scorer: 1 the product path (fp64 MFMA b + X M^T; the linear forms with a
 * finite M only, anything else fails the create), 2 the plain path (one
 * thread per row and class, j ascending; every model type), 0 auto: the
 * product where it is allowed.  cyc_nbmodel_path reports the path (1 or 2).
 *
 * cyc_nbmodel_score_dev: raw (nrows x numClasses), prob (exp(raw - max) /
 * sum_c exp(raw_c - max)), pred (nrows; the first index of the largest raw
 * under >, from class 0, as fp64); any of the three may be NULL, not all.
 * Rows are checked first in a pass of their own: multinomial and complement
 * need values >= 0 (a NaN fails), bernoulli exactly 0 or 1, gaussian nothing.
 * The lowest offending row goes to *badRow (-1 when none; may be NULL) and the
 * call fails with the aggregate's message; the outputs are then undefined.
 * The call synchronizes the stream to read the flag (gaussian: it does not).
 *
 * Rows go through in chunks of cyc_nbmodel_chunk_rows = workspaceBytes / (8
 * numClasses) rows (0: 256 MiB; whole 256-row tiles when more than one; at
 * least 1), whose raw values live in the workspace when raw is NULL.  A
 * smaller workspace means more launches, never other bits.  Fixed-order sums,
 * no atomics on doubles: two calls on the same inputs give the same bits. */
typedef struct cyc_nbmodel_s* cyc_nbmodel;

int cyc_nbmodel_create(int32_t numClasses, int32_t numFeatures, int32_t modelType,
                       int64_t workspaceBytes, const double* b, const double* M, const double* V,
                       const double* ls, int32_t scorer, void* stream, cyc_nbmodel* model);
int cyc_nbmodel_destroy(cyc_nbmodel model);
int32_t cyc_nbmodel_path(cyc_nbmodel model);
int64_t cyc_nbmodel_chunk_rows(cyc_nbmodel model);
int cyc_nbmodel_score_dev(cyc_nbmodel model, const double* X, int64_t nrows, double* raw,
                          double* prob, double* pred, int64_t* badRow, void* stream);

/* ------------------------------------------------------ BisectingKMeans
 * mllib/clustering/BisectingKMeans.scala's inner iteration and
 * BisectingKMeansModel's descent over row-major fp64 rows (nrows x
 * numFeatures, nrows < 2^31), Euclidean measure.  The level logic and the tree
 * are host code (cycloneml_amd/bisecting_kmeans.py).
 *
 * State.  Every row has an int32 slot, a compact id of the cluster it sits in
 * (slot, device, nrows; NULL: every row in slot 0); the caller keeps the slot
 * <-> node index map.  table (HOST, 3 numSlots int32) holds per slot
 * (leftNew, rightNew, keepNew): the new slots of the children on offer, -1 for
 * an absent one, and the new slot of a row that is offered none.  New slots 0
 * .. numChildren - 1 are the children: row c of centers (numChildren x
 * numFeatures, device) and cnorm (its Vectors.norm, device).  keepNew is -1 or
 * >= numChildren; a slot has a child or a keepNew.  numChildren <=
 * cyc_bkm_max_children.
 *
 * cyc_bkm_step_dev writes newSlot (device, nrows; may be slot itself): the
 * child picked by DistanceMeasure.findClosest (:318-340, no statistics) over
 * [left, right] with xnorm (device, cyc_row_norms_dev) -- the bound (c.norm -
 * x.norm)^2 < best decides whether a center's Vectors.sqdist (j ascending,
 * unfused) is looked at, and it wins only under <, so ties go left -- the only
 * child when one is on offer, else keepNew.  Only rows with two children on
 * offer are loaded.  A slot outside [0, numSlots) is never an index: the row
 * keeps it and the call fails (rule 3).
 *
 * Summary (count and sums both non-NULL, device; else both NULL).  Per child
 * c, ADDED into count (int64, numChildren) and sums (fp64, numChildren (2 +
 * numFeatures): [wsum | sumSq | sum (numChildren x numFeatures)]): the rows
 * that picked c, the sum of w, of (xnorm xnorm) w and of w x (w: device, nrows,
 * or NULL for 1).  Buffers of several calls (or ranks) merge by addition.  sum
 * is taken in row order within a child: chunks of cyc_bkm_chunk_rows rows,
 * folded in order; wsum and sumSq by one fixed tree per chunk, the chunks in
 * order.  The root's summary is the call with one slot, table (0, -1, -1) and
 * one child.
 *
 * check != 0 also checks the rows: xnorm finite (rule 1), w finite and > 0
 * (rule 2).  The lowest offending row and its rule go to *badRow / *badRule
 * (-1 / 0 when none; either may be NULL) and the call fails naming it; the
 * outputs are then undefined.  The call synchronizes the stream to read the
 * flag.
 *
 * cyc_bkm_predict_dev: the tree as HOST int32 arrays of numNodes entries, node
 * 0 the root: numChildren (0, 1 or 2), firstChild (the children are
 * firstChild, firstChild + 1; above the node's own index) and leafIndex (>= 0
 * at a leaf); centers (numNodes x numFeatures, device).  From the root a row
 * goes to the child of the smaller sqdist(child, x), the first on a tie, down
 * to a leaf: pred (int32, device) is its leafIndex, cost (fp64, device, may be
 * NULL) that last sqdist (a tree of one leaf: sqdist(root, x)).  It does not
 * synchronize.
 *
 * workspaceBytes (0: 256 MiB) bounds the summary's chunk partials:
 * cyc_bkm_chunks_per_launch chunks go through per launch (more launches when
 * it is smaller, never other bits; at least one chunk).  cyc_bkm_tile_rows
 * (rows per workgroup of the assign step and the descent) and
 * cyc_bkm_panel_cols (columns staged in LDS at a time) report the tiling.
 * fp64 throughout, fixed-order sums, no atomics on doubles: two calls on the
 * same inputs give the same bits. */
typedef struct cyc_bkm_plan_s* cyc_bkm_plan;

int cyc_bkm_plan_create(int32_t numFeatures, int64_t workspaceBytes, cyc_bkm_plan* plan);
int cyc_bkm_plan_destroy(cyc_bkm_plan plan);
int64_t cyc_bkm_tile_rows(cyc_bkm_plan plan);
int64_t cyc_bkm_panel_cols(cyc_bkm_plan plan);
int64_t cyc_bkm_chunk_rows(cyc_bkm_plan plan);
int64_t cyc_bkm_chunks_per_launch(cyc_bkm_plan plan);
int64_t cyc_bkm_max_children(cyc_bkm_plan plan);
int cyc_bkm_step_dev(cyc_bkm_plan plan, const double* X, const double* xnorm, const double* w,
                     int64_t nrows, const int32_t* slot, int32_t numSlots, const int32_t* table,
                     int32_t numChildren, const double* centers, const double* cnorm,
                     int32_t* newSlot, int64_t* count, double* sums, int32_t check,
                     int64_t* badRow, int32_t* badRule, void* stream);
int cyc_bkm_predict_dev(cyc_bkm_plan plan, const double* X, int64_t nrows, int32_t numNodes,
                        const int32_t* firstChild, const int32_t* numChildren,
                        const int32_t* leafIndex, const double* centers, int32_t* pred,
                        double* cost, void* stream);

/* --------------------------------------------------------- DecisionTree
 * One tree of ml/tree/impl/RandomForest.scala over row-major fp64 rows (nrows x
 * numFeatures, nrows < 2^31), continuous features: the binned rows, a level's
 * per-node histogram, the routing of rows to the children, and the model's
 * descent.  The split candidates, the split search and the tree are host code
 * (cycloneml_amd/tree.py).  A plan holds numFeatures (1 .. cyc_dt_max_features),
 * numClasses (1 .. 1024; 0: regression, the variance statistics) and the
 * workspace.
 *
 * cyc_dt_check_dev: the lowest row with a NaN feature (rule 1; +-inf is
 * legal), a label that is no integer in [0, numClasses) -- regression: not
 * finite -- (rule 2), or a weight that is not finite and >= 0 (rule 3; w may be
 * NULL) goes to *badRow / *badRule (-1 / 0 when none; either may be NULL) and
 * the call fails naming it.  It synchronizes the stream.
 *
 * cyc_dt_bin_dev: thresholds (HOST, numFeatures x 255, a feature's first
 * numSplits[f] entries ascending) and numSplits (HOST, int32) give image
 * (device, uint8, nrows x numFeatures): the number of the feature's thresholds
 * strictly below the value, so a value equal to threshold i gets bin i.
 *
 * State.  Every row has an int32 slot (device, nrows), a compact id of the node
 * it sits in; -1 is the skip slot of rows parked in leaves.  cyc_dt_route_dev
 * rewrites slot in place from table (HOST, 4 numSlots int32: feature, splitBin,
 * leftNew, rightNew per slot; feature < 0: parked): image[row][feature] <=
 * splitBin goes to leftNew, else rightNew; a parked slot's rows, and a slot
 * outside [0, numSlots), get -1.
 *
 * cyc_dt_histogram_dev: nodeOf (HOST, numSlots int32) names per slot its node 0
 * .. numNodes - 1 of this call (numNodes <= cyc_dt_max_nodes) or -1; slot NULL:
 * every row in slot 0.  hist (device, numNodes x numFeatures x numBins x
 * cyc_dt_num_stats, fp64) is SET to the sums over each node's rows at
 * [feature][image byte]: classification stat[label] += w and stat[numClasses]
 * += 1; regression w, w y, (w y) y, 1.  Rows of other slots are not loaded; an
 * image byte >= numBins is never an index.  A node's rows are added in row
 * order in runs of cyc_dt_run_rows rows and the runs folded in order;
 * workspaceBytes (0: 256 MiB) holds cyc_dt_runs_per_launch runs' partials (more
 * launches when it is smaller, never other bits; at least one run).  Buffers
 * of several ranks merge by addition.
 *
 * cyc_dt_predict_dev: the tree as HOST arrays of numNodes entries, node 0 the
 * root: feature and threshold of an internal node, firstChild (-1 at a leaf;
 * the children are firstChild, firstChild + 1, above the node's own index) and
 * leafIndex (0 .. numLeaves - 1 at a leaf); leafPred (HOST, numLeaves) and
 * leafRaw (HOST, numLeaves x numClasses, may be NULL).  x[feature] <= threshold
 * goes to firstChild.  Outputs (device, each may be NULL): leaf (int32), pred
 * (fp64), raw (nrows x numClasses) and prob (raw over its sum taken in class
 * order; raw itself when the sum is 0).  It does not synchronize.
 *
 * fp64 throughout, fixed-order sums, no atomics on doubles: two calls on the
 * same inputs give the same bits. */
typedef struct cyc_dt_plan_s* cyc_dt_plan;

int cyc_dt_plan_create(int32_t numFeatures, int32_t numClasses, int64_t workspaceBytes,
                       cyc_dt_plan* plan);
int cyc_dt_plan_destroy(cyc_dt_plan plan);
int64_t cyc_dt_max_features(void);
int64_t cyc_dt_max_nodes(void);
int64_t cyc_dt_run_rows(void);
int64_t cyc_dt_num_stats(cyc_dt_plan plan);
int64_t cyc_dt_runs_per_launch(cyc_dt_plan plan, int32_t numBins);
int cyc_dt_check_dev(cyc_dt_plan plan, const double* X, const double* y, const double* w,
                     int64_t nrows, int64_t* badRow, int32_t* badRule, void* stream);
int cyc_dt_bin_dev(cyc_dt_plan plan, const double* X, int64_t nrows, const double* thresholds,
                   const int32_t* numSplits, uint8_t* image, void* stream);
int cyc_dt_route_dev(cyc_dt_plan plan, const uint8_t* image, int64_t nrows, int32_t* slot,
                     int32_t numSlots, const int32_t* table, void* stream);
int cyc_dt_histogram_dev(cyc_dt_plan plan, const uint8_t* image, const double* y, const double* w,
                         int64_t nrows, const int32_t* slot, int32_t numSlots,
                         const int32_t* nodeOf, int32_t numNodes, int32_t numBins, double* hist,
                         void* stream);
int cyc_dt_predict_dev(cyc_dt_plan plan, const double* X, int64_t nrows, int32_t numNodes,
                       const int32_t* feature, const double* threshold, const int32_t* firstChild,
                       const int32_t* leafIndex, int32_t numLeaves, const double* leafPred,
                       const double* leafRaw, int32_t* leaf, double* pred, double* raw,
                       double* prob, void* stream);

/* --------------------------------------------------------- RandomForest
 * numTrees bagged trees of ml/tree/impl/RandomForest.scala grown level by level
 * over ONE binned image (cyc_dt_check_dev / cyc_dt_bin_dev above), every node
 * over its own subset of numSubset features.  A plan holds numFeatures,
 * numClasses (0: regression) and the workspace, as a DecisionTree plan does.
 * numTrees <= cyc_rf_max_trees.
 *
 * State (device, tree-major).  bag: numTrees x nrows uint8, the times tree t
 * drew row r (NULL: every row once).  slot: numTrees x nrows int32, the compact
 * id of the node row r sits in in tree t, -1: parked.  Per-tree host tables are
 * concatenated: tree t's entries are slotStart[t] .. slotStart[t + 1] (HOST,
 * int32, one more entry than trees, slotStart[0] = 0).
 *
 * cyc_rf_bag_dev: bag[t][r] = the number of table entries <= u, u = the top 53
 * bits of mix(seed, 0, t, rowOffset + r); table (HOST, tableLen <= 255 uint64
 * <= 2^53, ascending) holds floor(cdf_k 2^53).  mix(seed, stream, tree, index) =
 * fin(fin(fin(seed + G) + G (2 tree + stream + 1)) + G (index + 1)) mod 2^64,
 * fin = splitmix64's finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >>
 * 27, z *= 0x94D049BB133111EB, z ^= z >> 31), G = 0x9E3779B97F4A7C15.
 *
 * cyc_rf_route_dev: cyc_dt_route_dev's rule for every (tree, row) in one launch,
 * table (HOST, 4 slotStart[numTrees] int32) addressed through slotStart.
 *
 * cyc_rf_histogram_dev: one call covers the nodes 0 .. numNodes - 1 (<=
 * cyc_rf_max_nodes) of the trees [tree0, tree1), (tree1 - tree0) nrows <= 2^31 -
 * 1.  bag and slot are the WHOLE arrays (tree 0's first); slotStart (tree1 -
 * tree0 + 1 entries) and nodeOf (slotStart's last entry many, node or -1 per
 * slot) belong to the range; a node may be named by slots of one tree only.
 * nodeFeat (HOST, numNodes x numSubset int32 in [0, numFeatures); NULL: numSubset
 * = numFeatures, every feature in order) lists each node's features.  hist
 * (device, numNodes x numSubset x numBins x cyc_rf_num_stats) is SET to the sums
 * over each node's pairs at [j][image[row][nodeFeat[node][j]]]: classification
 * stat[label] += count w and stat[numClasses] += count, regression iw = count w:
 * iw, iw y, (iw y) y, count, count = bag[t][row].  A pair whose slot sits out or
 * whose count is 0 is never loaded.  A node's pairs are cut in row order into
 * runs of cyc_rf_run_rows and every run into cyc_rf_sub_runs(numSubset) fixed
 * slices; the partials are folded in (run, slice) order.  workspaceBytes holds
 * cyc_rf_runs_per_launch runs' partials: a smaller one means more launches,
 * never other bits, and neither do the tree range or the grouping of nodes.
 *
 * cyc_rf_predict_dev: the trees as concatenated HOST arrays in
 * cyc_dt_predict_dev's form, tree t's nodes at nodeStart[t] .. nodeStart[t + 1]
 * with firstChild and leafIndex local to the tree, its leaves at leafStart[t] ..;
 * leafValue (HOST, fp64): per leaf numClasses votes (class weights over their
 * sum; zeros for a leaf without weight) or the regression prediction.  Outputs
 * (device, each may be NULL): leaf (nrows x numTrees int32, the tree's own leaf
 * index), raw (nrows x numClasses, the votes added in tree order), prob (raw over
 * its sum taken in class order, raw itself when the sum is 0), pred (the first
 * largest raw; regression: the predictions added in tree order over numTrees).
 * A classifier's prob and pred need raw.  It does not synchronize. */
typedef struct cyc_rf_plan_s* cyc_rf_plan;

int cyc_rf_plan_create(int32_t numFeatures, int32_t numClasses, int64_t workspaceBytes,
                       cyc_rf_plan* plan);
int cyc_rf_plan_destroy(cyc_rf_plan plan);
int64_t cyc_rf_max_trees(void);
int64_t cyc_rf_max_nodes(void);
int64_t cyc_rf_run_rows(void);
int64_t cyc_rf_num_stats(cyc_rf_plan plan);
int64_t cyc_rf_sub_runs(int32_t numSubset);
int64_t cyc_rf_runs_per_launch(cyc_rf_plan plan, int32_t numSubset, int32_t numBins);
int cyc_rf_bag_dev(cyc_rf_plan plan, int64_t nrows, int32_t numTrees, int64_t rowOffset,
                   uint64_t seed, const uint64_t* table, int32_t tableLen, uint8_t* bag,
                   void* stream);
int cyc_rf_route_dev(cyc_rf_plan plan, const uint8_t* image, int64_t nrows, int32_t numTrees,
                     int32_t* slot, const int32_t* slotStart, const int32_t* table, void* stream);
int cyc_rf_histogram_dev(cyc_rf_plan plan, const uint8_t* image, const double* y, const double* w,
                         const uint8_t* bag, int64_t nrows, const int32_t* slot, int32_t tree0,
                         int32_t tree1, const int32_t* slotStart, const int32_t* nodeOf,
                         int32_t numNodes, int32_t numSubset, const int32_t* nodeFeat,
                         int32_t numBins, double* hist, void* stream);
int cyc_rf_predict_dev(cyc_rf_plan plan, const double* X, int64_t nrows, int32_t numTrees,
                       const int32_t* nodeStart, const int32_t* leafStart, const int32_t* feature,
                       const double* threshold, const int32_t* firstChild,
                       const int32_t* leafIndex, const double* leafValue, int32_t* leaf,
                       double* raw, double* prob, double* pred, void* stream);

/* ------------------------------------------------- GradientBoostedTrees
 * What ml/tree/impl/GradientBoostedTrees.scala's boost does between two trees,
 * and the descent of a boosted ensemble.  The trees are grown by the
 * RandomForest entry points above (one tree per iteration on the current
 * residuals); the loop and the models are host code (cycloneml_amd/gbt.py).  A
 * plan holds numFeatures and the scratch of the calls.
 *
 * cyc_gbt_update_dev: one tree as HOST arrays of numNodes entries in
 * cyc_dt_predict_dev's breadth-first form (feature, firstChild; -1 at a leaf)
 * with value[i] the prediction of leaf node i.  The rows come EITHER as the
 * binned image (uint8, nrows x numFeatures; X NULL) with splitBin[i] the split
 * of internal node i as a bin (0 .. 254; the position of its threshold among
 * the feature's thresholds): image byte <= splitBin goes to firstChild, the
 * byte compared unsigned; OR as fp64 rows X (image NULL) with threshold[i]:
 * x[feature] <= threshold goes to firstChild.  Per row, every operation rounded
 * once and unfused: F = pred + value treeWeight, pred (device, in/out) <- F,
 *   loss 0 squared   g = -2 (y - F),                    e = (y - F)(y - F)
 *   loss 1 absolute  g = y - F < 0 ? 1 : -1,             e = |y - F|
 *   loss 2 logistic  g = (-4 y) / (1 + exp((2 y) F)),    e = 2 log1pExp(-(2 y) F)
 * resid (device, may be NULL) <- -g, and sums (device, 2 doubles) is SET to the
 * sum of e w and the sum of w (w NULL: every weight 1.0).  The sums have one
 * fixed order: 256 consecutive rows through a binary tree (stride 128 .. 1),
 * the workgroups' partials t, t + 256, .. added in order by thread t of one
 * workgroup and those 256 through the same tree.  A tree of at most
 * cyc_gbt_lds_nodes nodes is staged in LDS, a larger one is read from global
 * memory; the bits do not depend on it.  Two calls give the same bytes.
 *
 * cyc_gbt_predict_dev: numTrees (<= cyc_gbt_max_trees) trees as concatenated
 * HOST arrays, tree t's nodes at nodeStart[t] .. nodeStart[t + 1], firstChild
 * local to the tree, leafIndex and value per NODE (read at leaves), treeWeights
 * (HOST, numTrees).  margin = sum over t of value_t treeWeights[t], from 0.0 in
 * tree order, each product rounded before its add, whatever the tiling of the
 * trees in LDS.  Outputs (device, each may be NULL): leaf (nrows x numTrees
 * int32), margin, raw = (-margin, margin), prob = (1 - p, p) with p = 1 / (1 +
 * exp(-2 margin)), pred (classifier != 0: margin > 0 ? 1 : 0, else margin); raw
 * and prob need classifier != 0.  Both calls upload the tree from the plan's
 * own host copy and wait for that upload; they do not wait for the kernels. */
typedef struct cyc_gbt_plan_s* cyc_gbt_plan;

int cyc_gbt_plan_create(int32_t numFeatures, cyc_gbt_plan* plan);
int cyc_gbt_plan_destroy(cyc_gbt_plan plan);
int64_t cyc_gbt_lds_nodes(void);
int64_t cyc_gbt_max_trees(void);
int cyc_gbt_update_dev(cyc_gbt_plan plan, const uint8_t* image, const double* X, int64_t nrows,
                       int32_t numNodes, const int32_t* feature, const int32_t* splitBin,
                       const double* threshold, const int32_t* firstChild, const double* value,
                       double treeWeight, int32_t loss, const double* y, const double* w,
                       double* pred, double* resid, double* sums, void* stream);
int cyc_gbt_predict_dev(cyc_gbt_plan plan, const double* X, int64_t nrows, int32_t numTrees,
                        const int32_t* nodeStart, const int32_t* feature,
                        const double* threshold, const int32_t* firstChild,
                        const int32_t* leafIndex, const double* value, const double* treeWeights,
                        int32_t classifier, int32_t* leaf, double* margin, double* raw,
                        double* prob, double* pred, void* stream);

/* ------------------------------------------------------------------ ALS */
/* One half-step of ml/recommendation/ALS.scala's computeFactors
 * (NormalEquation.add per rating, CholeskySolver.solve per destination id)
 * and the model's predict, 1 <= rank <= 64.
 *
 * A side (cyc_als_side_create) is the ratings grouped by destination id as a
 * device CSR: rowptr (int64, m + 1), colidx (int32 source ids in [0, nsrc)),
 * values (float32 ratings, nnz); duplicate pairs stay separate entries.  The
 * three arrays are BORROWED: they stay alive and unchanged until
 * cyc_als_side_destroy.  Creation checks the structure on the device
 * (rowptr[0] == 0, rowptr non-decreasing, rowptr[m] == nnz, every colidx in
 * range; a violation fails with "requirement failed: ..." before anything
 * gathers through the arrays), counts each row's positive ratings and builds
 * the table of segments (at most cyc_als_segment ratings of one row each)
 * that every later solve walks.  It synchronizes the stream.
 *
 * cyc_als_solve_dev: Y (nsrc x rank float32, row-major) are the source
 * factors.  Row u, each rating (i, r) in order, fp64: da = (double) Y[i],
 * ata += c da da^T, atb += b da.  Explicit: c = 1, b = r, numExplicits = the
 * row's rating count.  implicitPrefs: c1 = alpha |r|, c = c1, b = 1 + c1 where
 * r > 0 and 0 elsewhere, numExplicits counts r > 0, and ata starts from YtY =
 * sum_i da_i da_i^T over all nsrc source rows (yty: rank x rank fp64, full
 * symmetric, from cyc_als_yty_dev; NULL: computed by the call).  Then ata's
 * diagonal += regParam numExplicits, a Cholesky solve in fp64, X[u] (m x rank
 * float32) = (float) solution.  present (m bytes) is 1 where the row has
 * ratings; a row without ratings gets a zero factor and 0.  *info (device
 * int64) is -1, or the lowest row whose factorization met a pivot that is not
 * positive (that row's factor is zero; the other rows are solved as usual).
 * The call does not synchronize: read info after the stream has run.
 *
 * cyc_als_predict_dev: out[p] = sdot(rank, U[users[p]], V[items[p]]) in fp32,
 * the products added left to right, unfused; NaN where an id is negative, at
 * or past its count, or marked absent (a NULL mask: every id present).
 *
 * cyc_als_recommend_dev: ALSModel.recommendForAll and the subset forms, a
 * fused score + top-num pass.  S (nsrcRows x rank float32) are the source
 * factors, D (ndst x rank float32) the destination factors; srcPresent /
 * dstPresent are their presence masks (NULL: every id present).  srcIds (m
 * int32) names the requested source rows, in any order and with repeats; NULL
 * means rows 0 .. m - 1 (then m <= nsrcRows).  For requested row u and every
 * PRESENT destination j, score(u, j) = ((0.0f + S[u,0] D[j,0]) + S[u,1] D[j,1])
 * + ... in fp32, unfused: the same bits as cyc_als_predict_dev gives for the
 * pair.  Candidates are ordered by score descending under
 * java.lang.Float.compare (NaN is canonical, 0x7fc00000, and above everything;
 * -0.0 is below +0.0); EQUAL SCORES GO TO THE LOWER DESTINATION ID.  Spark
 * leaves ties to its bounded queue's internals; this total order is this
 * library's own, so the answer does not depend on tiles, splits or merge order
 * and two calls give the same bytes.  Row u of ids (m x num int32) and scores
 * (m x num float32) holds the first num candidates in that order; with fewer
 * than num present destinations the tail is -1 / NaN.  A source id that is
 * negative, at or past nsrcRows, or absent gives a whole row of -1 / NaN, and
 * nothing is gathered through it (the rule of cyc_als_predict_dev).
 * workspace: at least cyc_als_recommend_workspace(m, ndst, rank, num) device
 * bytes, 8-byte aligned, the call's alone until the stream has run it.  The
 * call keeps no state and does not synchronize.  rank outside 1 .. 64, num < 1
 * or above cyc_als_recommend_max_num() (128) and a short workspace fail with
 * "requirement failed: ..." before any launch.
 * The shape queries (pure functions of their arguments, the same on every
 * device): cyc_als_recommend_src_tile() source rows per workgroup;
 * cyc_als_recommend_dst_tile(rank) destination rows per LDS tile (0 for a bad
 * rank); cyc_als_recommend_lds_num() the greatest num whose lists are kept
 * in LDS (above it they live in the workspace: another path, the same
 * result); cyc_als_recommend_splits(m, ndst) the number of pieces the
 * destination range is cut into and cyc_als_recommend_span(m, ndst) their
 * length (split s covers [s span, min(ndst, (s + 1) span))).
 *
 * fp64 MFMA, fixed-order sums, no floating-point atomics: two calls on the
 * same inputs give the same bits. */
typedef struct cyc_als_side_s* cyc_als_side;

int cyc_als_segment(void);
int cyc_als_side_create(const int64_t* rowptr, const int32_t* colidx, const float* values,
                        int64_t m, int64_t nnz, int64_t nsrc, int32_t rank, void* stream,
                        cyc_als_side* side);
int cyc_als_side_destroy(cyc_als_side side);
int cyc_als_yty_dev(cyc_als_side side, const float* Y, double* yty, void* stream);
int cyc_als_solve_dev(cyc_als_side side, const float* Y, double regParam, int32_t implicitPrefs,
                      double alpha, const double* yty, float* X, uint8_t* present, int64_t* info,
                      void* stream);
int cyc_als_predict_dev(const float* U, const uint8_t* userPresent, int64_t numUsers,
                        const float* V, const uint8_t* itemPresent, int64_t numItems, int32_t rank,
                        const int32_t* users, const int32_t* items, int64_t n, float* out,
                        void* stream);
int cyc_als_recommend_src_tile(void);
int cyc_als_recommend_dst_tile(int32_t rank);
int cyc_als_recommend_max_num(void);
int cyc_als_recommend_lds_num(void);
int64_t cyc_als_recommend_splits(int64_t m, int64_t ndst);
int64_t cyc_als_recommend_span(int64_t m, int64_t ndst);
int64_t cyc_als_recommend_workspace(int64_t m, int64_t ndst, int32_t rank, int32_t num);
int cyc_als_recommend_dev(const float* S, const uint8_t* srcPresent, int64_t nsrcRows,
                          const int32_t* srcIds, int64_t m, const float* D,
                          const uint8_t* dstPresent, int64_t ndst, int32_t rank, int32_t num,
                          int32_t* ids, float* scores, void* workspace, int64_t workspaceBytes,
                          void* stream);

/* ------------------------------------------------ summarizer pre-pass */
/* The first pass of LogisticRegression.train (LogisticRegression.scala:
 * 511-516, Summarizer.getClassificationSummarizers, ml/stat/Summarizer.scala:
 * 228-241) and of RowMatrix/colStats, and the StandardScaler transform of
 * trainImpl (:957-965), over a device-resident shard.
 *
 * SummarizerBuffer (Summarizer.scala:428-770): a buffer is
 * cyc_summarizer_buffer_len(F) = 8 F + 5 doubles (device): per column mean,
 * m2n, m2, l1, weightSum, nnz, max, min (structure of arrays), then count,
 * totalWeightSum, weightSquareSum, a flag set when a row's weight failed
 * `require(weight >= 0.0)` (:472) and that weight.  The rows are cut into
 * partitions (dense: rows_per_partition rows; CSR: the row blocks of the CSC
 * copy), each partition's buffer is add()-ed row by row in the reference's
 * order and the partitions are merged (:562-617) in order.  Buffers of
 * several shards merge with cyc_summarizer_merge_dev, in the given order.
 * metrics (9 x F doubles): mean, variance, std, sum, numNonzeros, max, min,
 * normL2, normL1 (:622-769); count and weightSum are buf[8F], buf[8F+1]. */
int64_t cyc_summarizer_buffer_len(int32_t numFeatures);
int cyc_summarizer_dense_dev(const double* X, const double* weights, int64_t n, int32_t F,
                             int64_t rows_per_partition, double* buf, void* stream);
int cyc_summarizer_csr_dev(cyc_csc csc, const double* weights, double* buf, void* stream);
int cyc_summarizer_merge_dev(int32_t F, const double* bufs, int64_t count, double* out,
                             void* stream);
int cyc_summarizer_metrics_dev(int32_t F, const double* buf, double* metrics, void* stream);
/* MultiClassSummarizer (ml/stat/MultiClassSummarizer.scala:30-98) of the
 * labels: hist[max_classes] = per-class weight sums (classes >= max_classes
 * are counted in max_label only), *invalid = countInvalid, *max_label = the
 * largest valid label (-1: none; numClasses = max_label + 1; call again with
 * a larger max_classes, at most 8192, when it does not fit).  All device. */
int cyc_label_summarizer_dev(const double* labels, const double* weights, int64_t n,
                             int64_t rows_per_partition, int32_t max_classes, double* hist,
                             int64_t* invalid, int32_t* max_label, void* stream);
/* StandardScaler transform with scale only (StandardScaler.scala:261-283),
 * in place: dense values(i) *= scale(i); CSR values(k) *= scale(indices(k)). */
int cyc_scale_columns_dense_dev(double* X, int64_t n, int32_t F, const double* scale,
                                void* stream);
int cyc_scale_columns_csr_dev(const int32_t* colidx, double* vals, int64_t nnz,
                              const double* scale, void* stream);
/* InstanceBlock.blokifyWithMaxMemUsage (ml/feature/Instance.scala:146-187;
 * Matrices.fromVectors's dense-or-sparse choice, Matrices.scala:1010-1049)
 * over one partition's device rows -- dense X (n x F) OR CSR (rowptr, vals),
 * weights optional (null = all 1): starts[0..nblocks] (int64, capacity n + 1,
 * starts[nblocks] = n), dense[b] = 1 iff block b is stored dense, *nblocks;
 * all device.  maxMemUsage <= 0 -> "requirement failed: maxMemUsage > 0".
 * Replaces the per-partition iterator the reference runs on the executor. */
int cyc_blokify_dev(const double* X, const int64_t* rowptr, const double* vals,
                    const double* weights, int64_t n, int32_t F, int64_t maxMemUsage,
                    int64_t* starts, uint8_t* dense, int64_t* nblocks, void* stream);

/* ------------------------------------------- resident datasets (host API) */
/* Layer 2 for a JVM shim: a library-owned HBM copy of one
 * partition's rows, appended once from host blocks (an InstanceBlock's
 * row-major values / CSR arrays, labels and weights, Instance.scala:39-106),
 * then evaluated per iteration with host-pointer model inputs and
 * host-pointer aggregator outputs (ADDED to, like `add`).  The calls wrap
 * the _dev entry points above on the dataset's own stream and return after
 * the outputs are on the host.  Row norms (KMeans) and the CSC copy (sparse
 * binary LR) are built on first use and rebuilt after an append.
 *   cyc_kmeans_iter             KMeans.scala:287-311 (one partition of a Lloyd
 *                               iteration: statistics, findClosest, sums)
 *   cyc_logreg_*_eval           RDDLossFunction.scala:56-70's seqOp over the
 *                               partition's blocks
 *   cyc_gramian, cyc_col_sums   RowMatrix.scala:130-161, :163-220, :456
 * Dense and CSR datasets serve every entry point (CSR Gramian / column sums:
 * the sparse spr rows densified in chunks, cyc_gramian_accumulate_csr_dev). */
typedef struct cyc_dataset_s* cyc_dataset;

int cyc_dataset_dense_create(int32_t numFeatures, int64_t capacity_rows, int has_labels,
                             int has_weights, cyc_dataset* out);
int cyc_dataset_csr_create(int32_t numFeatures, int64_t capacity_rows, int64_t capacity_nnz,
                           int has_labels, int has_weights, cyc_dataset* out);
int cyc_dataset_destroy(cyc_dataset ds);
int64_t cyc_dataset_rows(cyc_dataset ds);
/* X: rows x numFeatures row-major.  labels / weights: `rows` doubles, required
 * iff the dataset was created with them. */
int cyc_dataset_append_dense(cyc_dataset ds, const double* X, const double* labels,
                             const double* weights, int64_t rows);
/* rowptr: rows+1 entries (any base: rowptr[0] is subtracted), colidx in
 * [0, numFeatures), sorted within a row as in SparseVector. */
int cyc_dataset_append_csr(cyc_dataset ds, const int64_t* rowptr, const int32_t* colidx,
                           const double* vals, const double* labels, const double* weights,
                           int64_t rows);

/* centers: k x d row-major.  sums[k*d] += sum w*x, wsum[k] += sum w,
 * cost[0] += sum w*cost; assign_opt (may be NULL) receives the rows'
 * cluster indices. */
int cyc_kmeans_iter(cyc_dataset ds, const double* centers, int32_t k, double* sums, double* wsum,
                    double* cost, int32_t* assign_opt);
/* The same for a DistanceMeasure (CYC_DISTANCE_*, cyc_kmeans_plan_set_distance
 * _measure); center_norms (host, k; may be NULL = computed) are the centers'
 * VectorWithNorm norms -- with COSINE 1.0 after an update (DistanceMeasure.
 * scala:477-483), which the distances divide by. */
int cyc_kmeans_iter_measure(cyc_dataset ds, int32_t measure, const double* centers,
                            const double* center_norms, int32_t k, double* sums, double* wsum,
                            double* cost, int32_t* assign_opt);
int cyc_logreg_binary_eval(cyc_dataset ds, const double* coef, int fitIntercept, int fitWithMean,
                           const double* scaledMean, double* grad, double* lossSum,
                           double* weightSum);
int cyc_logreg_multinomial_eval(cyc_dataset ds, int32_t numClasses, const double* coef,
                                int fitIntercept, int fitWithMean, const double* scaledMean,
                                double* grad, double* lossSum, double* weightSum);
/* U: packed upper n(n+1)/2 (column-major); mean_opt centers the rows. */
/* The other block aggregators over the resident rows, same conventions as
 * cyc_logreg_*_eval (host model in, host state out; grad / lossSum /
 * weightSum accumulate): LinearSVC's HingeBlockAggregator (dim F +
 * fitIntercept), LinearRegression's LeastSquaresBlockAggregator (dim F;
 * inverseStd required) and HuberBlockAggregator (dim F + fitIntercept + 1),
 * AFTSurvivalRegression's AFTBlockAggregator (dim F + 2; the dataset's
 * weights are the censors). */
int cyc_svc_hinge_eval(cyc_dataset ds, const double* coef, int fitIntercept,
                       const double* scaledMean, double* grad, double* lossSum,
                       double* weightSum);
int cyc_linreg_least_squares_eval(cyc_dataset ds, const double* coef, const double* inverseStd,
                                  int fitIntercept, double labelStd, double labelMean,
                                  const double* scaledMean, double* grad, double* lossSum,
                                  double* weightSum);
int cyc_linreg_huber_eval(cyc_dataset ds, const double* params, int fitIntercept, double epsilon,
                          const double* scaledMean, double* grad, double* lossSum,
                          double* weightSum);
int cyc_aft_eval(cyc_dataset ds, const double* coef, int fitIntercept, const double* scaledMean,
                 double* grad, double* lossSum, double* weightSum);
int cyc_gramian(cyc_dataset ds, const double* mean_opt, double* U);
int cyc_col_sums(cyc_dataset ds, double* sums);

/* ----------------------------------------- the aggregation step (RCCL) */
/* One process per GPU, one communicator per process.
 * Replaces RDD.treeAggregate (core/src/main/scala/org/apache/spark/rdd/
 * RDD.scala:1210-1269: seqOp per partition, foldByKey tree levels
 * :1244-1250, driver fold :1267), KMeans' reduceByKey + collectAsMap
 * (mllib/clustering/KMeans.scala:308-311) and the DoubleAccumulator cost by
 * ONE in-place fp64 sum of the flat aggregator state per iteration
 * (gradient | loss | weight, sums | weights | cost, packed Gramian), and
 * TorrentBroadcast of the model (SparkContext.scala:1524) by a broadcast.
 * Rank 0 makes the id with cyc_comm_unique_id and ships the 128 bytes to
 * every rank out of band (e.g. the Spark driver's broadcast); every rank then
 * calls cyc_comm_init with the same id, world size and its own rank and
 * device (collective: it returns once all ranks have joined; it sets the
 * calling thread's current device).  The sum order across ranks is RCCL's
 * (fixed for a topology), like Spark's completion-order fold it is not the
 * 1-GPU order: results agree to ~1e-15 relative.
 * _dev forms: device buffers, enqueued on `stream`.  Host forms: staged
 * through the communicator's own device buffer and stream, synchronous. */
#define CYC_COMM_ID_BYTES 128
typedef struct cyc_comm_s* cyc_comm;
int cyc_comm_unique_id(unsigned char* id /* CYC_COMM_ID_BYTES */);
int cyc_comm_init(const unsigned char* id, int32_t rank, int32_t world, int32_t device,
                  cyc_comm* out);
int cyc_comm_destroy(cyc_comm comm);
int cyc_comm_rank(cyc_comm comm, int32_t* rank, int32_t* world);
int cyc_allreduce_sum_dev(cyc_comm comm, double* buf, int64_t count, void* stream);
int cyc_allreduce_max_dev(cyc_comm comm, double* buf, int64_t count, void* stream);
int cyc_broadcast_dev(cyc_comm comm, double* buf, int64_t count, int32_t root, void* stream);
/* recv[r*count .. (r+1)*count) = rank r's send (the summarizer buffers,
 * merged in rank order by cyc_summarizer_merge_dev) */
int cyc_allgather_dev(cyc_comm comm, const double* send, double* recv, int64_t count,
                      void* stream);
int cyc_allreduce_sum(cyc_comm comm, double* host_buf, int64_t count);
int cyc_broadcast(cyc_comm comm, double* host_buf, int64_t count, int32_t root);

/* ------------------------------------------------------- LIBSVM input */
/* MLUtils.loadLibSVMFile's parse (mllib/util/MLUtils.scala:91-151:
 * parseLibSVMFile, parseLibSVMRecord, computeNumFeatures) on the host, in
 * parallel over line ranges, straight into CSR arrays for the device
 * (KMeansExample's and the sparse LR configs' input format).  Rows keep file
 * order; labels/values are bit-identical to Double.parseDouble; a bad record
 * returns CYC_ERR_INVALID_ARG with the reference's require text.
 * numFeatures <= 0: max(last index of each row, 0) + 1.  Host-only. */
typedef struct cyc_libsvm_s* cyc_libsvm;
int cyc_libsvm_parse(const char* text, int64_t len, int32_t numFeatures, int nthreads,
                     cyc_libsvm* out);
int cyc_libsvm_load_file(const char* path, int32_t numFeatures, int nthreads, cyc_libsvm* out);
int cyc_libsvm_sizes(cyc_libsvm h, int64_t* n, int64_t* nnz, int32_t* numFeatures);
/* host copies: labels[n], rowptr[n+1], colidx[nnz], values[nnz] (any may be NULL) */
int cyc_libsvm_copy(cyc_libsvm h, double* labels, int64_t* rowptr, int32_t* colidx,
                    double* values);
/* device copies (same shapes), synchronous on the stream */
int cyc_libsvm_upload(cyc_libsvm h, double* labels, int64_t* rowptr, int32_t* colidx,
                      double* values, void* stream);
int cyc_libsvm_destroy(cyc_libsvm h);

#ifdef __cplusplus
}
#endif

#endif /* CYCLONE_H */
