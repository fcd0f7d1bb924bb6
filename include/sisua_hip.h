/* sisua_hip.h -- C-ABI of the MI355X-native SISUA training hot path.
 *
 * The reference (trungnt13/sisua) has no FFI: its hot path is reached through the
 * Python class surface SingleCellModel.fit/predict/encode/decode
 * (sisua/models/single_cell_model.py:67-306), which hands every minibatch to
 * odin-ai / TensorFlow.  This library replaces everything below that class
 * surface.  Each entry point cites the reference interface it replaces; the
 * ctypes binding a maintainer would add is sisua_amd/_hip.py (see
 * INTEGRATION.md).
 *
 * Conventions: plain pointers and sizes, no torch / HIP types.  Every function
 * returns 0 on success and a negative smx_status otherwise; smx_last_error()
 * returns a thread-local message.  The caller owns every host buffer, the
 * library owns every device buffer.  One host thread (process) per GPU; all
 * kernels of a model run on one HIP stream owned by the model.  Host arrays
 * are dense row-major with LOGICAL shapes (the padded HBM layout is private).
 *
 * THE ROWS CONVENTION.  An entry that takes a host matrix of n rows x n_genes
 * columns "dense or CSR" takes it as the four arguments (x, indptr, cols, vals),
 * in this order, EXACTLY ONE of x / indptr non-NULL (SMX_ERR_INVALID before any
 * device work otherwise):
 *   dense  x float32 [n][n_genes], row-major; indptr = cols = vals = NULL;
 *   CSR    x = NULL; indptr int64 [n + 1] (absolute offsets: row i is entries
 *          indptr[i] .. indptr[i + 1] - 1 of cols / vals, never decreasing, at
 *          most n_genes entries per row), cols int32 (sorted within a row, each
 *          < n_genes), vals float32.
 * Both forms of the same counts give the same result bits.  In the model entries
 * the dense pointer is called host_x; a second matrix of a call (a target, the
 * original counts, a validation set) is the same four arguments under a prefix
 * (t_, o_, v_).
 */
#ifndef SISUA_HIP_H_
#define SISUA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_ABI_VERSION 22
#define SMX_MAX_LAYERS 8
#define SMX_MAX_LABELS 4

typedef enum {
  SMX_OK = 0,
  SMX_ERR_INVALID = -1,   /* bad argument / shape / state            */
  SMX_ERR_HIP = -2,       /* a HIP runtime call failed               */
  SMX_ERR_NOMEM = -3,
  SMX_ERR_COMM = -4,      /* RCCL not loadable or a collective failed */
  SMX_ERR_NAN = -5        /* terminate_on_nan (configs/base.yaml:59)  */
} smx_status;

/* Model families: sisua/models/vae.py:15-16 (VAE), dca.py:13-28, scvi.py:20-171,
 * vae.py:19-44 (SISUA = VAE + label heads; MISA = SISUA with mixture label heads, vae.py:47-98). */
/* SMX_MODEL_SCALE: scale.py:13-49 (SCALE, Xiong et al. 2019): VAE whose prior over z is a trainable mixture of
 * n_components diagonal Gaussians, KL term by one-sample Monte Carlo (`analytic=False`).  With label heads (n_labels > 0) it
 * is SCALAR (scale.py:52-59: SCALE + SISUA's semi-supervised heads). */
/* SMX_MODEL_FVAE: fvae.py:9-18 (FVAE / SemiFVAE; Kim & Mnih 2018): VAE + a discriminator on z whose logit estimates the
 * total correlation; the VAE's tensors follow -ELBO + gamma TC, the discriminator's tensors its own classification loss
 * (z against z with every dimension permuted over the minibatch), both in the same step.  Label variables (behind the
 * observed outputs; SMX_LABEL_ONEHOT, 32 classes in all) make it the semi-supervised form: one logit per class of every
 * variable, TC logit = the logsumexp of all of them, each variable's masked cross-entropy under the softmax of its own. */
typedef enum { SMX_MODEL_VAE = 0, SMX_MODEL_DCA = 1, SMX_MODEL_SCVI = 2, SMX_MODEL_SISUA = 3, SMX_MODEL_SCALE = 4,
               SMX_MODEL_FVAE = 5,
               SMX_MODEL_SCALE_TRIL = 6 /* SCALE with covariance = 'tril' / 'full' (scale.py:28,35): a lower-triangular scale factor per
                                          component -- prior/scale is [n_components * latent_dim][latent_dim] (diag = softplus + 1e-5) */,
               SMX_MODEL_SCALE_POST = 7 /* scale.py:26,38-47 read literally: the latent POSTERIOR is a mixture of n_components (2 .. min(latent_dim,
                                          8)) diagonal Gaussians from a (1 + 2 n_components) * latent_dim wide latent head (logits in the first columns
                                          of plane 0 | locations | raw scales), standard-normal prior, Monte-Carlo KL; no prior tensors */ } smx_model_kind;
/* Count likelihoods selected by RVmeta.posterior (configs/base.yaml:32-40,
 * data/_single_cell_base.py:518-533). */
/* SMX_LLK_MSE: RVmeta(dim, 'mse') (the reference's tests/test_singlecell_models.py:82-91, 97-100): a deterministic output, ONE
 * parameter plane (the mean), log p(x) := -mean_g (x - mean)^2 -- exactly minus tf.losses.mse.  No marginal-likelihood scoring. */
/* SMX_LLK_BERNOULLI: RVmeta(dim, 'bernoulli') (binarised peak matrices: SCALE / SCALAR's scATAC input), ONE plane of logits l:
 * log p(x) = sum_g x l - softplus(l) (TFP Bernoulli.log_prob, defined for any x in [0, 1]).
 * SMX_LLK_NORMAL: RVmeta(dim, 'normal' / 'gaussian' / 'diag') (real-valued inputs: log-normalised expression, CLR protein panels), TWO
 * planes -- loc m | raw scale s, sigma = softplus(s + softplus^-1(1)): log p(x) = sum_g -z^2 / 2 - log sigma - log(2 pi) / 2, z = (x - m) / sigma.
 * Both are normalised densities WITHOUT the count constant -sum_g lgamma(x + 1): they score (marginal likelihood, posterior_llk) like the
 * count posteriors.  The same element forms as SMX_LABEL_BERNOULLI / SMX_LABEL_NORMAL. */
typedef enum { SMX_LLK_NB = 0, SMX_LLK_ZINB = 1, SMX_LLK_NBD = 2, SMX_LLK_ZINBD = 3, SMX_LLK_MSE = 4, SMX_LLK_BERNOULLI = 5,
               SMX_LLK_NORMAL = 6 } smx_likelihood;
/* Label heads of SISUA (vae.py:19-44): NB (ADT counts), one-hot categorical (cell types); of MISA (vae.py:47-98): every
 * label dimension a mixture of label_components (2..4) negative binomials (SMX_LABEL_MIXNB) or, for continuous labels, normals
 * (SMX_LABEL_MIXGAUSS, 'mixgaussian', vae.py:86-92); SMX_LABEL_MIXTRIL ('mixtril', the class's docstring example vae.py:58): ONE
 * mixture of label_components full-covariance Gaussians over the whole label vector (lower-triangular scale factors; label_dim <= 64;
 * the head then has label_components * (2 + label_dim) planes); SMX_LABEL_MIXZINB: MISA(zero_inflated=True), vae.py:76-84 -- the
 * components of SMX_LABEL_MIXNB zero-inflated, a fourth group of label_components gate-logit planes. */
/* SMX_LABEL_NBD / ZINB / ZINBD: the remaining count posteriors of RVmeta as heads (vae.py:30 "'onehot'/'nbd'/'nb'"; the second OUTPUT of
 * tests/test_singlecell_models.py:133-134 is 'nbd'): planes as for the gene output -- (mean, dispersion) through softplus / softplus1,
 * (log total_count, logits, gate logits), (mean, dispersion, gate logits). */
/* SMX_LABEL_BERNOULLI ('bernoulli'): every label dimension its own binary variable (binarised protein markers, multi-label), ONE
 * plane of logits l: log p(y) = y l - softplus(l), defined for any y in [0, 1] (a probability matrix trains too).
 * SMX_LABEL_NORMAL ('normal' / 'gaussian' / 'diag'): an independent normal per label dimension, TWO planes -- loc m | raw scale s,
 * sigma = softplus(s + softplus^-1(1)) ([3P-recall] odin's softplus1: the scale activation of the latents and of SMX_LABEL_MIXGAUSS's
 * components). */
typedef enum { SMX_LABEL_NB = 0, SMX_LABEL_ONEHOT = 1, SMX_LABEL_MIXNB = 2, SMX_LABEL_MIXGAUSS = 3, SMX_LABEL_MIXTRIL = 4, SMX_LABEL_MIXZINB = 5,
               SMX_LABEL_NBD = 6, SMX_LABEL_ZINB = 7, SMX_LABEL_ZINBD = 8, SMX_LABEL_BERNOULLI = 9, SMX_LABEL_NORMAL = 10 } smx_label_likelihood;
/* Activations: smx_config.latent_activation (dca: RELU or LINEAR) and the hidden layers of each network (smx_set_activation: all of them).
 * SMX_ACT_LEAKY_RELU has slope 0.2 (tf.nn.leaky_relu), SMX_ACT_ELU alpha 1, SMX_ACT_SELU the Keras constants lambda = 1.0507009873554805,
 * alpha = 1.6732632423543772. */
typedef enum { SMX_ACT_RELU = 0, SMX_ACT_LINEAR = 1, SMX_ACT_LEAKY_RELU = 2, SMX_ACT_ELU = 3, SMX_ACT_SELU = 4, SMX_ACT_TANH = 5,
               SMX_ACT_SIGMOID = 6, SMX_ACT_SOFTPLUS = 7 } smx_activation;
/* Networks of smx_set_activation. */
typedef enum { SMX_NET_ENCODER = 0, SMX_NET_DECODER = 1, SMX_NET_LIBRARY_ENCODER = 2 } smx_network;
/* Optimiser rules (smx_set_optimizer; tf.keras 2.x Adam, SGD, RMSprop, Adagrad, Adamax). */
typedef enum { SMX_OPT_ADAM = 0, SMX_OPT_SGD = 1, SMX_OPT_RMSPROP = 2, SMX_OPT_ADAGRAD = 3, SMX_OPT_ADAMAX = 4 } smx_optimizer;
#define SMX_OPT_MAX_HP 4
/* Step-dependent weights (smx_set_schedule): the target, and the kind of schedule with its parameters in this order.
 *   interpolations of the KL weight ([3P-recall] odin's `interpolation`, re-exported by the reference), keyed by the model's step:
 *     SMX_SCHED_CONST         vmax
 *     SMX_SCHED_LINEAR        vmin, vmax, norm, cyclical (0 / 1), delayIn, delayOut
 *     SMX_SCHED_POWER         vmin, vmax, norm, cyclical, delayIn, delayOut, power
 *     SMX_SCHED_COSINE        vmin, vmax, norm, cyclical, delayIn, delayOut
 *   tf.keras 2.x learning-rate schedules, keyed by the optimiser's own count step - t0 (smx_get_optimizer):
 *     SMX_SCHED_EXP_DECAY     initial_learning_rate, decay_steps, decay_rate, staircase (0 / 1)
 *     SMX_SCHED_INVTIME_DECAY initial_learning_rate, decay_steps, decay_rate, staircase (0 / 1)
 *     SMX_SCHED_PIECEWISE     boundaries[k], values[k + 1]  (n = 2 k + 1)
 *     SMX_SCHED_POLY_DECAY    initial_learning_rate, decay_steps, end_learning_rate, power, cycle (0 / 1)
 *     SMX_SCHED_COSINE_DECAY  initial_learning_rate, decay_steps, alpha
 * Either kind may serve either target. */
typedef enum { SMX_SCHED_BETA = 0, SMX_SCHED_LR = 1 } smx_schedule_target;
typedef enum { SMX_SCHED_CONST = 0, SMX_SCHED_LINEAR = 1, SMX_SCHED_POWER = 2, SMX_SCHED_COSINE = 3, SMX_SCHED_EXP_DECAY = 4,
               SMX_SCHED_INVTIME_DECAY = 5, SMX_SCHED_PIECEWISE = 6, SMX_SCHED_POLY_DECAY = 7, SMX_SCHED_COSINE_DECAY = 8 } smx_schedule_kind;

/* Constructor arguments of SingleCellModel / SCVI / SISUA / DeepCountAutoencoder
 * (single_cell_model.py:74-97, scvi.py:33-48, vae.py:40-44, dca.py:16-28) plus
 * the optimiser block of configs/base.yaml:45-50. */
typedef struct {
  int32_t abi_version;                 /* must be SMX_ABI_VERSION */
  int32_t model;                       /* smx_model_kind */
  int32_t likelihood;                  /* smx_likelihood */
  int32_t n_genes;                     /* G */
  int32_t latent_dim;                  /* D */
  int32_t n_enc, enc_units[SMX_MAX_LAYERS];
  int32_t n_dec, dec_units[SMX_MAX_LAYERS];
  int32_t n_encl, encl_units[SMX_MAX_LAYERS];   /* scvi library encoder */
  int32_t n_labels, label_dim[SMX_MAX_LABELS], label_llk[SMX_MAX_LABELS];
  int32_t label_components[SMX_MAX_LABELS];   /* SMX_LABEL_MIXNB / MIXGAUSS / MIXTRIL: mixture components (MISA n_components, vae.py:77) */
  /* outputs[1:] of the reference's constructors (single_cell_model.py:74-97; tests/test_singlecell_models.py:129-141
   * `VAE(outputs=[RVmeta(G, 'zinb'), RVmeta(P, 'nbd')])`; scvi.py:168-169 `pY = [p(d) for p in self.posteriors[1:]]`): a head with
   * label_observed[j] != 0 is a further OUTPUT variable -- fully observed (the label mask is not consulted), weight 1 instead of alpha,
   * its negative log-likelihood reported as smx_metrics.nllk_o.  Observed heads come first; any model kind but SMX_MODEL_FVAE /
   * SMX_MODEL_SCALE_POST takes them (label heads proper keep their model-kind rule). */
  int32_t label_observed[SMX_MAX_LABELS];
  /* scvi.py:55-56,66-86,136-160 `dispersion` / `inflation` of the gene output: 0 = 'full' (a Dense head per cell and gene), 1 = 'share'
   * (no head: ONE trainable vector [n_genes] shared by every cell -- tensor out1/b resp. out2/b without out1/W resp. out2/W; theta = exp of
   * it, gate logits = it), 2 = 'single' (ONE trainable scalar for every cell and gene: out1/b resp. out2/b of one element).  SMX_MODEL_SCVI only. */
  int32_t scvi_dispersion, scvi_inflation;
  int32_t n_components;                /* SMX_MODEL_SCALE: components of the mixture prior (scale.py:27), 1..32 */
  /* RVmeta(latent_dim, 'mvntril') / 'tril': a full-covariance Gaussian posterior q(z|x) = N(mu, L L^T) (SMX_MODEL_VAE, SISUA, SCVI's z;
   * 1 <= latent_dim <= 32).  The latent head has 1 + latent_dim planes of width latent_dim: plane 0 mu, plane 1 + i row i of the raw factor
   * (L_ij = raw_ij for j < i, L_ii = softplus(raw_ii) + 1e-5, entries j > i inert).  z_scale outputs then hold the factor L
   * [batch, latent_dim, latent_dim] (row-major, zeros above the diagonal) instead of [batch, latent_dim].  0: the diagonal posterior. */
  int32_t latent_tril;
  int32_t disc_units, disc_layers;     /* SMX_MODEL_FVAE: hidden width / hidden layers of the discriminator (odin: 1000, 5) */
  float gamma, disc_leak;              /* SMX_MODEL_FVAE: weight of the TC term (6.0); leaky-ReLU slope (0.2) */
  int32_t batchnorm;                   /* NetConf.batchnorm */
  int32_t log_norm;                    /* single_cell_model.py:82 */
  int32_t latent_activation;           /* dca only */
  float dropout_enc, dropout_dec, input_dropout;
  float beta, alpha;                   /* base.yaml:6-7 */
  float clip_library;                  /* scvi.py:47 */
  float bn_momentum, bn_eps;
  float lr, adam_beta1, adam_beta2, adam_eps, clipnorm;
  int32_t max_batch;                   /* largest minibatch a step will see */
  uint64_t seed;                       /* Philox key (dropout masks, eps) */
} smx_config;

/* Scalars of one step, mean over the (global) minibatch; names follow the
 * reference's logged scalars (tutorials/notebook/...ipynb:238: loss, nllk_x, KLqp). */
typedef struct {
  float loss, nllk_x, nllk_y, kl, kl_l;
  float grad_norm_max;   /* largest per-tensor gradient norm before clipping */
  int32_t nan_flag;      /* non-zero if any of the above is not finite */
  int32_t step;          /* optimiser step count after this call */
  float tc, dtc_loss;    /* SMX_MODEL_FVAE: total-correlation estimate mean d(z); the discriminator's loss (0 otherwise) */
  float nllk_o;          /* the observed extra outputs (label_observed): -mean sum of their log-likelihoods (0 without them) */
} smx_metrics;

typedef struct smx_model smx_model;

/* ---- process / device ---------------------------------------------------- */
const char* smx_last_error(void);
int smx_abi_version(void);
/* Number of visible HIP devices (0 when there is no GPU). */
int smx_device_count(void);
/* Bind this process to a device.  Replaces `CUDA_VISIBLE_DEVICES='0'` (train.py:20). */
int smx_init(int device);
int smx_synchronize(void);

/* ---- model lifetime ------------------------------------------------------ */
/* SingleCellModel.__init__ (single_cell_model.py:74-101). Glorot-uniform weights
 * are NOT drawn here: the host sets them with smx_set_tensor (keeps init RNG on
 * the Python side, shared with the oracle). */
int smx_model_create(const smx_config* cfg, smx_model** out);
int smx_model_destroy(smx_model* m);

/* Manifest of trainable tensors, in oracle order (oracle/sisua_oracle.py:manifest). */
int smx_num_tensors(const smx_model* m);
int smx_tensor_info(const smx_model* m, int index, char* name, int name_cap, int32_t* rows, int32_t* cols);
/* which: 0 = parameters, 1 = gradients of the last step (after all-reduce, before
 * clipping), 2 = Adam m, 3 = Adam v.  Replaces save_weights/load_weights
 * (single_cell_model.py:283-306) and serves the parity tests.
 * Under the other rules of smx_set_optimizer, which = 2 / 3 are that rule's slots: sgd the momentum accumulator / - (no
 * slot at momentum 0), rmsprop mom / ms (mom unused at momentum 0), adagrad - / the accumulator, adamax m / u.  A slot a
 * rule does not use keeps whatever it holds and is not read. */
int smx_get_tensor(smx_model* m, int which, int index, float* host);
int smx_set_tensor(smx_model* m, int which, int index, const float* host);
/* Batch-norm moving statistics, layer order = oracle bn_manifest; which: 0 mean, 1 var. */
int smx_num_bn_layers(const smx_model* m);
int smx_get_bn(smx_model* m, int layer, int which, float* host, int32_t* width);
int smx_set_bn(smx_model* m, int layer, int which, const float* host);
int smx_get_step(const smx_model* m, int32_t* step);
int smx_set_step(smx_model* m, int32_t step);

/* ---- data ---------------------------------------------------------------- */
/* Upload the (already split / corrupted) cells x genes matrix once; it stays
 * resident in HBM (replaces the per-step tf.data H2D copy of
 * data/_single_cell_base.py:539-602).  X [n_cells, G] dense float32 (the
 * reference's on-disk format, data/utils.py:427-431).  labels[j] is
 * [n_cells, label_dim[j]] or NULL; library [n_cells,2] = (local_mean, local_var)
 * (:568-570) or NULL; label_mask [n_cells] 0/1 or NULL (:580-591).
 * cell_id_base offsets the Philox cell ids (rank shard offset). */
int smx_dataset_upload(smx_model* m, const float* X, int64_t n_cells, const float* const* labels,
                       const float* library, const uint8_t* label_mask, int64_t cell_id_base);
/* The same with the counts stored compactly as uint16 (every count must be <= 65535): half the
 * HBM footprint and half the gather traffic of the dense float32 memmap of the reference
 * (sisua/data/utils.py:401-452), identical results -- the kernels widen on load.  Labels stay float32. */
int smx_dataset_upload_u16(smx_model* m, const uint16_t* X, int64_t n_cells, const float* const* labels,
                           const float* library, const uint8_t* label_mask, int64_t cell_id_base);

/* Compact sparse store (the dense float32 memmap semantics of sisua/data/utils.py:401-452 over the
 * non-zeros only): the counts as CSR -- indptr [n_cells + 1] (indptr[0] = 0), then column indices (< n_genes) and
 * float32 values of the non-zeros row by row; 8 bytes per non-zero on the device.  Every pass expands its minibatch's
 * rows into a dense float32 tile first, so every result is bit-identical to the float32 store.  smx_dataset_library /
 * smx_dataset_corrupt need a dense store; input dropout too (its noise is keyed by the dense store's rows). */
int smx_dataset_upload_csr(smx_model* m, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells,
                           const float* const* labels, const float* library, const uint8_t* label_mask, int64_t cell_id_base);

/* The rank's shard of BASELINE.json configs[4] ("synthetic 1e6 cells x 20k genes log-normal counts"), generated ON the
 * device ("generated on-device per shard from (seed, rank)"; the reference's scaling test draws its matrix
 * with NumPy on the host, tests/test_scalability.py:22-27): n_cells rows of ONE virtual matrix whose entry (cell, gene) is
 * a function of (seed, global cell id = rank * n_cells + row, gene) only -- x = floor(LogNormal(mu_gene, 1)) kept with
 * probability `density` (0.14 leaves ~93 % zeros), capped at 65535, gene 0 >= 1.  storage_u16 != 0: the compact store
 * (40 GB for 1e6 x 20 000).  Replaces the resident matrix; no labels / library prior (VAE / DCA models).  Bit-for-bit the
 * oracle's generate_lognormal_rows up to exp() rounding at integer boundaries. */
/* A dense store (float32; uint16 with storage_u16 != 0, integer counts <= 65535) from cells given as CSR (layout as smx_dataset_upload_csr):
 * blocks of rows cross as CSR and are expanded into the store on the device, so the host never holds the dense matrix.  The store, its
 * row constants and every later result are those of smx_dataset_upload / smx_dataset_upload_u16 on the same counts. */
int smx_dataset_upload_csr_dense(smx_model* m, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells,
                                 const float* const* labels, const float* library, const uint8_t* label_mask, int64_t cell_id_base,
                                 int32_t storage_u16);
int smx_dataset_generate_lognormal(smx_model* m, uint64_t seed, int32_t rank, int64_t n_cells, int32_t storage_u16, double density);

int64_t smx_dataset_size(const smx_model* m);

/* Library-size statistics of the RESIDENT matrix, get_library_size (sisua/data/utils.py:231-263) as the
 * reference recomputes them after corrupt() (sisua/data/_single_cell_analysis.py:110): log_counts = log(sum_g x
 * + 1e-8) per cell, local_mean / local_var over cells.  Fills the resident [n_cells, 2] library prior with
 * (local_mean, local_var) and returns them in stats[0..1] (stats may be NULL). */
int smx_dataset_library(smx_model* m, float stats[2]);

/* apply_artificial_corruption(distribution='binomial') (sisua/data/utils.py:168-228; SingleCellOMIC.corrupt,
 * _single_cell_analysis.py:78-111) IN PLACE on the resident matrix: exactly floor(dropout * nnz) of the non-zero
 * entries, chosen without replacement, become Binomial(n = x, p = retain_rate).  The draws come from the Philox
 * counter RNG keyed by (seed, cell id, gene), not from NumPy's MT19937 stream: same law, order independent,
 * bit-identical to oracle/sisua_oracle.py:corrupt_philox (the host path sisua_amd.data.corrupt keeps the
 * reference's RandomState stream bit-exactly).  Refreshes the per-row likelihood constants; call
 * smx_dataset_library afterwards as the reference does.  Same argument checks as the reference: dropout in
 * [0, 1); no-op unless 0 < dropout < 1 or 0 < retain_rate < 1. */
int smx_dataset_corrupt(smx_model* m, double dropout, double retain_rate, uint64_t seed, int64_t* n_corrupted);

/* Read back rows of the resident matrix (tests / checkpoints): X [n_rows, n_genes], the per-row constant
 * sum_g lgamma(x+1) [n_rows], the library prior [n_rows, 2]; any output may be NULL. */
int smx_dataset_read(smx_model* m, int64_t row0, int64_t n_rows, float* X, float* row_const, float* library);

/* ---- the hot path -------------------------------------------------------- */
/* One optimiser step on the cells `row_ids` of the resident matrix: forward,
 * ELBO, backward, (all-reduce), per-tensor clipnorm, Adam.  Replaces one
 * iteration of the odin Trainer loop under SingleCellModel.fit
 * (single_cell_model.py:213-236).  `out` may be NULL (no host
 * sync).  batch <= cfg.max_batch. */
int smx_train_step(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out);
/* Same arithmetic, launched as one captured hipGraph (fixed batch size). */
int smx_train_step_graph(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out);
/* Queue `n_steps` steps whose row ids are order[s*batch .. (s+1)*batch); no host
 * sync between steps (order = NULL: the ids staged by smx_train_stage).  `out` (may be NULL) receives the last step's metrics; a non-finite loss or gradient
 * norm is reported through out->nan_flag with status SMX_OK (terminate_on_nan is the caller's decision). */
int smx_train_steps(smx_model* m, const int32_t* order, int32_t n_steps, int32_t batch, int use_graph,
                    smx_metrics* out);
/* The row ids of the NEXT smx_train_steps call made resident ahead of it: that call is then given order = NULL (same
 * n_steps and batch) and queues its steps without the host-to-device copy of the ids -- the minibatch schedule of an epoch is
 * input data like the matrix itself (an input pipeline's prefetch; single_cell_model.py:213-236 iterates a prepared
 * tf.data stream).  The staged ids serve ONE call. */
int smx_train_stage(smx_model* m, const int32_t* order, int32_t n_steps, int32_t batch);
/* ELBO scalars of EVERY step of the last smx_train_steps call, kept on the device while the steps ran (no host
 * sync between them): host [n_steps][8] = (loss, nllk_x, nllk_y, kl, kl_l, 0, 0, 0) per step, global-minibatch
 * means.  Feeds the per-epoch train_history of SingleCellModel.fit (tests/test_singlecell_models.py:28-32 of the
 * reference reads train_history['loss'] per epoch). */
int smx_metrics_history(smx_model* m, int32_t n_steps, float* host);
/* Validation loss: eval-mode forward (moving BN stats, no dropout) + ELBO, no
 * update (valid_freq loop of BetaVAE.fit). */
int smx_eval_step(smx_model* m, const int32_t* row_ids, int32_t batch, smx_metrics* out);
/* Monte-Carlo draws per cell of the later smx_train_step(_graph) / smx_train_steps / smx_eval_step calls
 * (SingleCellModel.fit(sample_shape), sisua/train.py:138,146; default 1).  A step of `batch` cells then runs on
 * n_draws x batch stacked rows, draw-major (row r = draw r / batch of cell r % batch): the encoder-side noise of
 * every row is its cell's (sample index 0), the draw-side noise (latent draws, the decoder's dropout) takes sample
 * index r / batch, and the ELBO scalars are means over cells and draws.  The row buffers grow to n_draws x
 * max_batch on first use; captured graphs are dropped whenever the count changes.  SMX_ERR_INVALID for
 * n_draws < 1, for FactorVAE / SemiFVAE with n_draws > 1 and for a data-parallel model (world > 1). */
int smx_set_train_draws(smx_model* m, int32_t n_draws);
/* The optimiser rule of the later training steps (the `optimizer:` key of configs/base.yaml:45-50, handed to the Keras optimiser
 * registry by the reference): rule = smx_optimizer, hp[n_hp] its hyper-parameters in this order (entries not given take the
 * tf.keras 2.x defaults in parentheses):
 *   SMX_OPT_ADAM      beta_1, beta_2, epsilon (smx_config.adam_beta1 / adam_beta2 / adam_eps -- the rule a model is created with)
 *   SMX_OPT_SGD       momentum (0), nesterov (0 / 1)
 *   SMX_OPT_RMSPROP   rho (0.9), momentum (0), epsilon (1e-7)
 *   SMX_OPT_ADAGRAD   initial_accumulator_value (0.1), epsilon (1e-7)
 *   SMX_OPT_ADAMAX    beta_1 (0.9), beta_2 (0.999), epsilon (1e-7)
 * Every epsilon must be a normal float32 (>= 2^-126), smx_config.adam_eps included: at 0 (or a denormal, whose reciprocal is inf) the update
 * makes 0 * inf = NaN of every tensor's zero padding.  SMX_ERR_INVALID otherwise, before any device work.
 * Every rule keeps smx_config.lr, the per-tensor clipnorm in front of the update and the tied-variable norm of SCALE.  The rule
 * starts FRESH, as a new Keras optimiser object does: its slots (smx_get_tensor which = 2 / 3) are set to 0 -- Adagrad's
 * accumulator to initial_accumulator_value -- and t0 = the model's step count now (smx_set_step first to record another); the
 * rule's step count is t = step + 1 - t0 (Adam's and Adamax's bias correction).  Captured graphs are dropped.  With opt_shard
 * the fresh slots are whole on every rank.  SMX_ERR_INVALID for an unknown rule, n_hp > SMX_OPT_MAX_HP or a value out of range. */
int smx_set_optimizer(smx_model* m, int32_t rule, const float* hp, int32_t n_hp);
/* The rule in force, its SMX_OPT_MAX_HP hyper-parameters (defaults filled in, unused entries 0) and t0; any output may be NULL. */
int smx_get_optimizer(const smx_model* m, int32_t* rule, float* hp, int32_t* t0);
/* The schedule of a step-dependent weight: target = smx_schedule_target, kind = smx_schedule_kind, params[n] as listed there.  The
 * default is SMX_SCHED_CONST at smx_config.beta / .lr.  The schedule is evaluated on the host in double and rounded once to float: each
 * smx_train_steps / smx_train_stage call uploads the (beta, lr) of its steps as a table beside the row ids, and every step -- eager or
 * a replayed graph -- reads its own entry on the device (StepState).  Eval passes (smx_eval_step) take beta at the model's step.
 * Learning rate: the rule's step size is taken from the scheduled value at step - t0.  Captured graphs stay valid.  SMX_ERR_INVALID for an
 * unknown target or kind, a wrong n, norm / decay_steps <= 0, negative delays, boundaries that do not increase, non-finite values. */
int smx_set_schedule(smx_model* m, int32_t target, int32_t kind, const double* params, int32_t n);
/* The schedule in force: kind, and its parameters into params[cap] (may be NULL); *n = their count (a piecewise schedule may hold more
 * than cap: *n tells). */
int smx_get_schedule(const smx_model* m, int32_t target, int32_t* kind, double* params, int32_t cap, int32_t* n);
/* Host evaluation of a schedule without a model or a device: out[i] = the float value at step first_step + i, i < count -- exactly what a
 * training step's table holds.  SMX_ERR_INVALID as smx_set_schedule. */
int smx_schedule_eval(int32_t kind, const double* params, int32_t n, int64_t first_step, int32_t count, float* out);
/* The activation of every hidden layer of one network: net = smx_network, act = smx_activation.  The default is SMX_ACT_RELU.  Latent and
 * head layers, DCA's latent activation and the FactorVAE discriminator keep theirs.  Activations have no parameters: the tensor list does
 * not change.  Layers other than ReLU take the general forms of the BatchNorm / activation launches; the fused forms that build ReLU in
 * (latent-sample and gradient fronts, the paired first layers, the activation epilogues of the products) are not used for them.  Captured
 * graphs are dropped.  SMX_ERR_INVALID for an unknown network or activation, or SMX_NET_LIBRARY_ENCODER on a model without one. */
int smx_set_activation(smx_model* m, int32_t net, int32_t act);

/* Eval-mode forward for predict/encode/decode (single_cell_model.py:119-211):
 * writes distribution parameters into caller-owned buffers (any may be NULL).
 * Input cells: row_ids into the resident matrix, or host_x [batch,G] when
 * row_ids == NULL (host_library [batch,2] for scvi).  sample_index selects the
 * Monte-Carlo draw of eps.  Outputs: z_mean/z_scale/z_sample [batch,D];
 * l_mean/l_scale/l_sample [batch] (scvi); x_params [k,batch,G] planes in
 * likelihood order (nb/zinb: log total_count, logits, gate logits;
 * nbd/zinbd: mean, dispersion, gate logits -- already activated);
 * y_params[j] [batch, ky*P_j] raw head outputs (ky = 2 NB: log total_count | logits; 1 one-hot: logits; 3 C mixture of
 * C NB: C mixture logits | C log total_counts | C logits, each P_j wide). */
int smx_forward(smx_model* m, const int32_t* row_ids, const float* host_x, const float* host_library,
                int32_t batch, int32_t sample_index, int32_t training, float* z_mean, float* z_scale,
                float* z_sample, float* l_mean, float* l_scale, float* l_sample, float* x_params,
                float* const* y_params);

/* n_samples Monte-Carlo draws of one batch in ONE call: SingleCellModel.predict(sample_shape=n) as
 * Posterior._initialize uses it (sisua/analysis/posterior.py:172-182, sample_shape = 10).  The encoders run once (eval
 * mode); draw s re-samples the latents with Philox sample index s and decodes -- the same draws as n_samples calls of
 * smx_forward(sample_index = s), and the same numbers to rounding (a host batch's draws are decoded as rows of one pass,
 * as in smx_predict; bit for bit with flag "stacked_scoring" = 0 and for resident rows).  z_mean / z_scale [batch, D] and l_mean / l_scale [batch] once; z_samples
 * [n_samples, batch, D]; l_samples [n_samples, batch]; x_params [n_samples, k, batch, n_genes]; y_params[j]
 * [n_samples, batch, ky * P_j].  Any output may be NULL. */
int smx_forward_samples(smx_model* m, const int32_t* row_ids, const float* host_x, const float* host_library, int32_t batch,
                        int32_t n_samples, float* z_mean, float* z_scale, float* z_samples, float* l_mean, float* l_scale,
                        float* l_samples, float* x_params, float* const* y_params);

/* SingleCellModel.predict(inputs, sample_shape, batch_size) over a whole host matrix in ONE call
 * (sisua/models/single_cell_model.py:153-211: "predict on minibatches then return a single distribution by
 * concatenation").  The n_cells host rows (host_library [n_cells, 2] for scvi) are walked in minibatches of `batch`
 * (<= max_batch; the last one may be smaller) and every result is written straight to its final place:
 * z_mean / z_scale [n_cells, D]; l_mean / l_scale [n_cells]; z_samples [n_samples, n_cells, D]; l_samples
 * [n_samples, n_cells]; x_params [n_samples, k, n_cells, n_genes]; y_params[j] [n_samples, n_cells, ky * P_j].  Same draws
 * as smx_forward_samples batch by batch (draw s uses Philox sample index s; the noise of a cell is keyed by its index
 * within its minibatch, as there); the same numbers bit for bit at one draw, to rounding with several (their decodes
 * then run as rows of one pass, flag "stacked_scoring").  Any output may be NULL.  The rows (host_x, indptr, cols,
 * vals): the rows convention above -- CSR rows are expanded on the device into the tile a dense chunk is re-pitched
 * into, their likelihood constants from the same launch, and chunks are cut by non-zeros as well as by cells. */
int smx_predict(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                int64_t n_cells, int32_t batch, int32_t n_samples, float* z_mean, float* z_scale, float* z_samples, float* l_mean,
                float* l_scale, float* l_samples, float* x_params, float* const* y_params);

/* The same walk over a host matrix, but what leaves the device is a STATISTIC of the gene output instead of its parameter planes -- what
 * the reference's callers ask of predict()'s result: `y.mean()`, `.variance()`, `.log_prob(x)` of the output distribution or of its
 * count distribution without the zero-inflation wrapper (sisua/analysis/posterior.py:187-255: 'reconstructed' / 'imputed').  The planes
 * are 4 k G bytes per cell and draw (24 KB at 1998 genes, zinb) and a fresh result array of that size is first-touched by the copy;
 * a mean is a third of it, the mean over the draws 1 / (3 n_samples), a log_prob 4 bytes.  Same passes, same draws as smx_predict.
 *   stat 0 mean, 1 variance: out [n_samples, n_cells, n_genes];  2 mean averaged over the draws: out [n_cells, n_genes];
 *   stat 3 log_prob (summed over the genes: Independent(..., 1)): out [n_samples, n_cells], of the target rows or, without a target,
 *          of the input rows themselves;  count_only != 0: the count distribution (NB / NBD) of a zero-inflated output.
 * The rows, and the log_prob target (target, t_indptr, t_cols, t_vals; n_cells rows; at most one of target / t_indptr): the rows
 * convention. */
int smx_predict_stat(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                     int64_t n_cells, int32_t batch, int32_t n_samples, int32_t stat, int32_t count_only, const float* target,
                     const int64_t* t_indptr, const int32_t* t_cols, const float* t_vals, float* out);

/* POSTERIOR-PREDICTIVE SAMPLES of the gene output, drawn on the device from the parameter planes of the same walk (its stat 4; the passes
 * of a chunk run once): out [n_k, n_samples, n_cells, n_genes] float32, n_k independent draws x ~ p(x | planes) per Monte-Carlo draw, cell
 * and gene -- `y.sample(n_k)` of predict()'s result.
 *   nb / zinb: Poisson(Gamma(shape = exp(p0), scale = exp(p1))); nbd / zinbd: Poisson(Gamma(shape = theta, scale = mean / theta));
 *   zero-inflated: kept with probability 1 - sigmoid(p2), else 0 (count_only != 0: the count distribution, no gate);
 *   bernoulli: u < sigmoid(p0); normal: loc + softplus(raw + softplus^-1(1)) n; mse: the location itself.
 * Counter-based: a draw is a function of (seed, sample k, draw s, row of the input, gene) alone -- philox4x32_10 under the key `seed` with
 * the counter (gene, row, k, 96 | attempt << 8 | s << 16) -- so the batch size, the chunking and dense / CSR input change no bit.  Every
 * rejection loop is bounded (16 Gamma attempts, 24 Poisson attempts, then the proposal's mean / the rounded rate).  Count outputs are
 * non-negative integers in float32; a NaN parameter, or a Gamma-Poisson rate that is not finite, gives NaN.  n_cells < 2^32,
 * n_samples <= 65536.  The rows: the rows convention. */
int smx_predict_sample(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                       int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, uint64_t seed, int32_t n_k, float* out);

/* Stat 2 (the mean averaged over the draws) for n_sel gene columns only: out [n_cells, n_sel], column j = gene genes[j] (any order,
 * repeats allowed, each in 0 .. n_genes - 1) -- the same bits as those columns of smx_predict_stat's [n_cells, n_genes].  The rows: the rows
 * convention. */
int smx_predict_stat_cols(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals,
                          const float* host_library, int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const int32_t* genes,
                          int32_t n_sel, float* out);

/* IMPUTATION SCORES (sisua/analysis/imputation_benchmarks.py:102-127) of the matrix smx_predict_stat's stat 2 returns for host_x, the
 * CORRUPTED counts -- same passes, same draws -- against `original` [n_cells, n_genes], reduced on the device: with
 * d = |original - mean over the draws|,
 *   cell_median [n_cells]   np.median(d[i]): 0.5f * (lo + hi) of the row's two middle order statistics, NaN if the row holds a NaN;
 *   cell_changed [n_cells]  1 where sum(original[i]) != sum(host_x[i]) (both sums in float64: for integer counts with row sums below
 *                           2^24 this is the reference's float32 np.sum comparison), else 0;
 *   global_lohi [2]         the order statistics (NG - 1) / 2 and NG / 2 of all NG = n_cells x n_genes entries of d (64-bit ranks);
 *                           both NaN if any entry is NaN.
 * Every selection is exact (integer histograms of the float32 patterns; no float atomics): the results do not depend on the batch size,
 * the chunking or the input form.  The global selection's later levels read d kept on the device when n_cells x n_genes x 4 bytes fit
 * the knob "impute_keep_bytes" (default: half of the free device memory) and otherwise repeat the walk twice; same answer.
 * The input rows, and the original rows (original, o_indptr, o_cols, o_vals; n_cells rows): the rows convention, exactly one form each. */
int smx_predict_impute(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals, const float* host_library,
                       int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const float* original, const int64_t* o_indptr,
                       const int32_t* o_cols, const float* o_vals, float* cell_median, int32_t* cell_changed, float* global_lohi);

/* GENE x PROTEIN CORRELATION SUMS (SingleCellOMIC.get_correlation, sisua/data/_single_cell_analysis.py:1199-1245: pearsonr and spearmanr of
 * every pair) of the matrix smx_predict_stat's stat 2 returns -- same passes, same draws -- against P protein columns the caller has
 * prepared on the host: prot_rank2 [P][n_cells] int32, 2 x the average rank of each cell within the protein's column; prot_unit
 * [P][n_cells] float64, the column centred and scaled to unit norm.  Arguments as smx_predict_stat_cols; genes = NULL: every gene
 * (n_sel ignored).  For selected gene j, with a = 2 x the average ranks of its column x (float32; -0 ties with +0):
 *   sp_Sa, sp_Saa [n_sel]      sum a, sum a a             sp_Sab [n_sel][P]   sum a prot_rank2[p]     (int64, exact)
 *   pe_mean, pe_Sxx [n_sel]    mean x, sum (x - mean)^2   pe_Sxy [n_sel][P]   sum (x - mean) prot_unit[p]   (float64, two passes, in an
 *                                                                             order that is a function of n_cells alone)
 *   nonfinite [n_sel]          1 where the column holds a NaN or an infinity (its other outputs are then unspecified), else 0.
 * Spearman = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2)(N Sbb - Sb^2)), Pearson = Sxy / sqrt(Sxx).  Nothing depends on the batch size, the
 * chunking or the input form.  n_cells <= 2^20 (4 n_cells^3 < 2^63), else SMX_ERR_INVALID before any device work.  The kept columns, their
 * ranks and the sort arrays take 16 n_cells bytes per gene: as many genes at a time as fit the knob "correlate_keep_bytes" (default: half
 * of the free device memory), the walk being repeated once per such chunk -- same bits.  The rows: the rows convention. */
int smx_predict_correlate(smx_model* m, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals,
                          const float* host_library, int64_t n_cells, int32_t batch, int32_t n_samples, int32_t count_only, const int32_t* genes,
                          int32_t n_sel, const int32_t* prot_rank2, const double* prot_unit, int32_t P, int64_t* sp_Sa, int64_t* sp_Saa,
                          int64_t* sp_Sab, double* pe_mean, double* pe_Sxx, double* pe_Sxy, int32_t* nonfinite);

/* Decoder only (SingleCellModel.decode, single_cell_model.py:141-151; scvi.py:108-171):
 * z [batch,D] (and l [batch] for scvi) -> the same x_params / y_params as smx_forward,
 * eval mode. */
int smx_decode(smx_model* m, const float* z, const float* l, int32_t batch, float* x_params, float* const* y_params);

/* Importance-weighted marginal log-likelihood, the scoring path of Posterior.cal_marginal_llk ->
 * scm.marginal_log_prob(**Xs, sample_shape=100) (sisua/analysis/posterior.py:941-976): the encoder runs once,
 * then the n_samples draws (z of draw s from Philox sample index s) go through decoder, output head and forward-only
 * likelihood as rows of one pass (up to 16 384 rows at a time; flag "stacked_scoring" = 0: draw by draw) with
 * a running log-sum-exp per cell on the device.  mllk[batch] = log mean_s p(x|z_s) p(z_s) / q(z_s|x);
 * llk_mean[batch] = mean_s log p(x|z_s) (may be NULL).  Cells: row_ids into the resident matrix, or (row_ids = NULL) `batch` host rows in
 * the rows convention (+ host_library for scvi) -- never both. */
int smx_marginal_llk(smx_model* m, const int32_t* row_ids, const float* host_x, const int64_t* indptr, const int32_t* cols, const float* vals,
                     const float* host_library, int32_t batch, int32_t n_samples, float* mllk, float* llk_mean);

/* Posterior-predictive scoring, Posterior.cal_llk (sisua/analysis/posterior.py:919-938): the cells given by
 * row_ids / host_x are encoded once, then n_samples posterior draws are decoded and the output distribution is
 * scored against each target matrix (host [batch, n_genes]; a NULL entry = the input cells themselves) with a
 * running log-sum-exp over the draws on the device.  out[(t*2 + j)*batch + b] = logsumexp_s log p_j(target_t[b] |
 * z_s) - log n_samples, j = 0 the model's output distribution ("reconstructed"), j = 1 its count distribution
 * without the zero-inflation gate ("imputed", posterior.py:218-225; equals j = 0 for nb / nbd). n_targets <= 4. */
int smx_score_llk(smx_model* m, const int32_t* row_ids, const float* host_x, const float* host_library,
                  const float* const* targets, int32_t n_targets, int32_t batch, int32_t n_samples, float* out);

/* Test hook: inject noise for the NEXT step instead of Philox.  stream ids as in
 * oracle/sisua_oracle.py (STREAM_*); data [batch, width] holds eps values or
 * dropout multipliers.  smx_clear_noise() returns to Philox. */
int smx_set_noise(smx_model* m, int32_t stream, const float* data, int32_t batch, int32_t width);
int smx_clear_noise(smx_model* m);

/* ---- data parallel (one process per GPU) ---------------------------------- */
/* 128-byte RCCL unique id, created on rank 0 and handed to every rank by the
 * host (torch.distributed / a file store). */
int smx_comm_unique_id(uint8_t id[128]);
/* Join the communicator; afterwards every train step all-reduces the flat
 * gradient buffer (+ BN batch stats + metrics) once over xGMI.  The loss is scaled by 1 / (batch * world), so
 * the summed buffer holds the gradient of the GLOBAL minibatch mean; smx_get_tensor(which = 1) returns it.
 * On failure the model is left without a communicator (world 1) and SMX_ERR_COMM is returned. */
int smx_comm_init(smx_model* m, int rank, int world, const uint8_t id[128]);
int smx_comm_world(const smx_model* m);
int smx_comm_rank(const smx_model* m);
/* How an (eager) training step exchanges its gradients right now: 0 no collective (world 1), 1 ONE all-reduce of the flat buffer between
 * the backward pass and the optimiser (north star; RCCL or the tests' loopback), 2 the two-bucket chain -- the heads' gradients (3/4 of the
 * bytes) all-reduced, normed and applied on a communication stream beside the rest of the step, the front bucket all-reduced on the model's
 * stream --, 3 the hand-written exchange over IPC-mapped peer buffers, one bucket, ONE launch per all-reduce on the model's stream, 4 the
 * hand-written exchange's two-bucket form of round 4 (both buckets on the communication stream; only under the library's own rule). */
int smx_comm_form(const smx_model* m);
/* Ask for a form: 1, 2 or 3 as above (3 needs smx_comm_p2p_init, 1 / 2 a communicator), or 0 = the library's own rule (the hand-written
 * exchange whenever it is attached; two buckets from 3 MB of head gradients, SMX_DP_BUCKETS=1|2 overrides).  A COLLECTIVE call when it
 * asks for 2 (the heads' communicator is split off on first use): every rank, same order.  sisua_amd/parallel.py measures the available
 * forms on the job's own steps and sets the fastest on every rank (calibrate_forms); nothing asked = nothing measured. */
int smx_comm_set_form(smx_model* m, int form);
/* Flag "opt_shard" (smx_set_flag; off by default; data parallel, the chained form -- it is taken whenever the flag is set): the output and
 * label heads' optimiser state is SHARDED over the ranks -- reduce-scatter of their gradient bucket, per-tensor clipnorm + Adam on this rank's
 * 1 / world slice, all-gather of the updated parameters (the same wire bytes as the all-reduce; 1 / world of the optimiser's memory traffic).
 * Parameters stay replicated and bit-identical on every rank; a rank's gradient buffer (smx_get_tensor, which = 1) holds the heads' REDUCED
 * gradient inside its slice only, and the Adam MOMENTS of the heads outside a rank's slice go stale.  smx_opt_gather
 * (a collective: every rank calls it, between training calls) all-gathers both moments, after which smx_get_tensor(which = 2 | 3) of a head
 * tensor -- refused while stale -- returns the job's moments on every rank (checkpoints); smx_train_steps calls it itself in front of steps that will
 * not take the sharded chain (a captured graph, the flag switched off since).  RCCL or the loopback communicator; with the
 * hand-written exchange the flag is ignored (the all-reduce form runs). */
int smx_opt_gather(smx_model* m);
/* The same all-reduce as a hand-written two-shot exchange over peer-mapped buffers instead of RCCL (reduce-scatter
 * + all-gather of the flat buffer through HIP-IPC-mapped peer memory over xGMI; sums in rank order -- bitwise the same on every
 * rank): smx_comm_p2p_export allocates this rank's communication region and returns its two 64-byte IPC handles (the flat
 * gradient buffer | the region); the host gathers the `world` x 128 bytes in rank order (control plane) and hands them to
 * smx_comm_p2p_init, after which every training step's collective (and SyncBatchNorm's small ones) takes this path -- with or
 * without an RCCL communicator (call smx_comm_init first when both are wanted).  world <= 8 (one node).  Waits on peers are
 * bounded (SMX_P2P_TIMEOUT_S, 30 s): a timed-out wait marks the step void on every rank -- smx_train_step* / smx_eval_step return
 * SMX_ERR_COMM on every call with a metrics read-back until smx_comm_p2p_error has read (and cleared) the word; the Python Engine does
 * that when it raises.  Recovery: restore the last checkpoint on every rank, re-attach the communicator. */
int smx_comm_p2p_export(smx_model* m, int world, uint8_t handles[128]);
int smx_comm_p2p_init(smx_model* m, int rank, int world, const uint8_t* all_handles);
int smx_comm_p2p_error(smx_model* m, int32_t* error);
/* Measurement hook (bench.py, N > 1): the step's collective ALONE -- `iters` all-reduces of the (zeroed) flat gradient buffer
 * through whichever path the steps take (RCCL, the peer-to-peer exchange, the loopback communicator), timed with events on the
 * model's stream after three untimed calls; every rank must call it with the same `iters`.  us_per_call: this rank's average;
 * floats (may be NULL): the buffer's length.
 * The gradient buffer is scratch between steps: nothing of the model's state changes. */
int smx_comm_time_allreduce(smx_model* m, int iters, float* us_per_call, int64_t* floats);
/* Which communication library the process is bound to, and the HIP runtime both it and this library run on
 * (RCCL is resolved as the sibling of the loaded libamdhip64: ROCm's, or torch's bundled copy when torch was
 * imported first; SMX_RCCL_PATH overrides).  rccl_version: ncclGetVersion code.  Any output may be NULL. */
int smx_comm_library(char* rccl_path, int rccl_cap, char* hip_path, int hip_cap, int32_t* rccl_version);
/* SyncBatchNorm (SURVEY.md 8e caveat i; opt-in): BatchNorm statistics over the GLOBAL minibatch, as the
 * single-process reference computes them -- one extra all-reduce of [world][2][H] column statistics per
 * BatchNorm layer forward and one backward.  Off (default): per-replica statistics, ONE all-reduce per step.
 * Every rank must run the same batch size. */
int smx_comm_set_sync_bn(smx_model* m, int on);
/* Test hook: join n models of THIS process (one device; each driven by its own host thread) into a loopback
 * communicator -- rank i = models[i].  Their steps all-reduce through events + a summing kernel instead of RCCL,
 * so the world > 1 arithmetic of the step can be checked on a one-GPU box.  Eager launches only. */
int smx_comm_init_local(smx_model* const* models, int n);

/* ---- host-side helper ------------------------------------------------------ */
/* Visit order of one epoch under a streaming shuffle buffer of `buffer` cells (tf.data .shuffle(1000) after .cache,
 * before .batch: sisua/data/_single_cell_base.py:597-600): at step t the element picks[t] % len(buffer) leaves the
 * buffer and the next unseen cell takes its place.  picks[n_obs]: non-negative random integers from the caller's
 * generator (the stream that defines the order); out[n_obs] receives the cell indices.  No device work. */
int smx_shuffle_order(int32_t n_obs, int32_t buffer, const int64_t* picks, int32_t* out);

/* ---- developer knobs -------------------------------------------------------- */
/* Tile / split-K / share sweeps, A/B of launch forms and test hooks (e.g. "score_rows", "predict_stage_floats", "no_sq_partials",
 * "adam_wide_share") live in ONE registry instead of an environment variable each: smx_set_tuning sets a knob for the process,
 * smx_clear_tuning removes one (name = NULL or "": all); the environment variable SMX_TUNING="name=value,name=value" presets them
 * (the scripts under tools/).  docs/LAB_NOTES.md lists the knobs and their defaults; none of them is needed to USE the library -- the switches a user
 * may need are the environment variables of INTEGRATION.md section C.  A model's launch-form flags read "no_<flag>" when it is created. */
int smx_set_tuning(const char* name, double value);
int smx_clear_tuning(const char* name);

/* ---- code-path switches ---------------------------------------------------- */
/* The training step has two forms of several stages: the default wide / fused kernels and the separate-launch forms
 * they replaced (which eval, predict and the scoring paths always use).  name: "head_loss" (output product fused with
 * the likelihood), "front" (latent sample + first decoder product inside BatchNorm-forward), "bwd_front" (d h inside
 * BatchNorm-backward + the weight gradients grouped at the end), "head_bwd" (both backward products of the output
 * head in one launch), "wgrad" (minibatch-contracted weight gradients as the wide kernel), "scvi_fused" (scvi
 * training step: library latent + softmax-rate head + likelihood + their backward as one row-local launch,
 * scvi.py:88-171), "twin" (scvi: the first layers of the encoder and of the library encoder, and pairs of output
 * heads, side by side in one launch), "label_ride" (SISUA / MISA: the label heads' d d as extra slabs of the output
 * head's backward launch, their weight gradients in the grouped launch at the end), "act_epilogue" (layers without
 * BatchNorm and dropout, e.g. the FactorVAE discriminator: bias + activation and the activation's derivative in the
 * products' store paths), "stacked_scoring" (smx_marginal_llk, smx_score_llk and smx_predict with several draws: all
 * posterior draws of a batch as rows of ONE decoder pass, in the scoring calls the output head fused with the
 * likelihood; 0 = one decoder pass per draw; SMX_NO_STACKED_SCORING).
 * "head_fused" (wide panels -- at least 4096 genes, 128 decoder columns, at most 128 cells, no label heads: the output product, the
 * likelihood AND both backward products of the head as one launch that owns a tile of 32 genes from the raw weights to their
 * gradients, smx_headfused.hip; 0 = the fused head + the two wide backward kernels).
 * "head_sweep" (with "head_fused", one GPU, eager steps: clip + Adam of the heads' tensors -- 3/4 of the parameters at 20 000 genes -- as a
 * background sweep of a fixed number of workgroups on a second stream, between this step's output head and the next step's; every
 * smx_train_steps call ends with the sweep joined; 0 = riders of the backward chain + the optimiser launch; same bits either way).
 * "bf16x3": the training products of the output head (the fused head, both products of its backward, the first layer's
 * weight gradient) from bf16 MFMAs on operands split three ways in registers (f32 accuracy to one rounding of a product;
 * 0.375 of the f32 MFMAs' cycles, on the matrix pipe): 1 always, 0 never (exact f32 MFMAs), -1 (default) from the head's
 * width -- SMX_BF16X3 in the environment sets the same default.
 * value 1 = default form, 0 = separate launches.  Results agree to rounding;
 * used for A/B measurements and by the parity tests of both forms.  Defaults may also be set with SMX_NO_HEAD_LOSS /
 * SMX_NO_FRONT / SMX_NO_BWD_FRONT / SMX_NO_HEAD_BWD / SMX_NO_WGRAD / SMX_NO_SCVI_FUSED / SMX_NO_TWIN /
 * SMX_NO_LABEL_RIDE / SMX_NO_ACT_EPILOGUE in the environment. */
int smx_set_flag(smx_model* m, const char* name, int value);

/* ---- measurement ---------------------------------------------------------- */
/* HIP-event timing of one named kernel class inside eager steps, on the model's
 * stream.  kernel: "out_head" (the fused output product + likelihood; 8 idempotent launches per event pair),
 * "out_head_product" (the same kernel without the likelihood: what the fused kernel's time is compared with), "loss"
 * (the standalone likelihood kernel, flag head_loss = 0), "gemm_enc_fwd", "gemm_out_fwd", "gemm_out_bwd" (dW + dX of the head),
 * "gemm_enc_dw", "bn_fwd", "bn_bwd", "adam", "allreduce", "step", or "null" (an event pair around
 * nothing: the overhead to subtract from single-kernel timings).  "out_head@N" / "out_head_product@N" / "loss@N": N
 * launches per event pair instead of 8 (N = 1: the single launch rocprofv3's per-kernel duration is compared with).
 * Enable, run steps, read. */
int smx_timing_enable(smx_model* m, const char* kernel);
int smx_timing_read(smx_model* m, double* total_ms, int64_t* launches);
/* Algorithmic bytes (fwd+bwd loss kernel = (4+8k)G + 16D + 4 per cell). */
int64_t smx_loss_bytes_per_cell(const smx_model* m);
/* Algorithmic bytes of ONE launch of the fused output head (smx_headfused.hip: W_out + bias read, dW_out + db written, decoder output,
 * counts, d d, likelihood partials) when a training step of `batch` cells takes it -- a wide panel (>= 4096 genes), 128 decoder columns,
 * batch <= 128, no label heads --, else 0: bench.py's roofline entry at the C5 width. */
int64_t smx_head_fused_bytes(const smx_model* m, int32_t batch);
/* 1 when the model's LAST training step left the output head's dW / db to the decoder's BatchNorm-backward launch (a narrow panel, at most
 * 128 cells, the plain bf16 x 3 head, one GPU: DESIGN.md section 4; knob no_dw_late), else 0: the tests' check that this form is what ran. */
int32_t smx_head_dw_late(const smx_model* m);
/* How many steps of the model's LAST smx_train_steps call left their optimiser launch out: the next step's first launch -- the gathered
 * encoder product -- then updates its block of the first encoder matrix in registers, and riders of the forward launches apply the update in
 * place (eager steps of one GPU under Adam, every step of a call but its last: DESIGN.md section 4; knob no_lazy_adam).  The tests' check
 * that this form is what ran. */
int32_t smx_lazy_adam_steps(const smx_model* m);
/* How many steps of the model's LAST smx_train_steps call ran the decoder's BatchNorm-backward launch (carrying the output head's dW) and the
 * encoder's (with the d z product folded in) as ONE launch whose encoder workgroups wait inside it for the decoder's d pre-activation (one
 * decoder layer of 128 units, an encoder of at most 128, at most 128 cells, one GPU, eager untimed steps: DESIGN.md section 4; knob
 * no_bwd_seam).  A wait that gives up sets an error word: the next metrics read-back fails with a message naming the seam. */
int32_t smx_bwd_seam_steps(const smx_model* m);

/* ---- kernel-level entry points (parity tests of single kernels) ------------ */
/* Fused count log-likelihood forward+backward over host planes [k][B][G]:
 * llk[B] and grads [k][B][G] (d llk / d plane, unscaled).  direct != 0: planes
 * are (mean, dispersion, gate) (scvi.py:151-164). */
int smx_k_count_llk(int likelihood, int direct, const float* x, const float* planes, int32_t B, int32_t G,
                    float* llk, float* grads);
/* The optimiser launch by itself over caller-given tensors (per-tensor clipnorm + Adam, row a-16): n_tensors
 * tensors of sizes[i] floats, concatenated in params / grads / m / v (host arrays; params, m, v updated in
 * place).  step = the 1-based count t of this update (lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) is evaluated on the
 * device as in a training step).  norms[n_tensors] (may be NULL): gradient norms before clipping. */
int smx_k_adam(int32_t n_tensors, const int32_t* sizes, float* params, const float* grads, float* m, float* v,
               int32_t step, float lr, float beta1, float beta2, float eps, float clipnorm, float* norms);
/* The same launch under any rule of smx_set_optimizer (rule, hp[n_hp] as there): m / v are the rule's slots 2 / 3 (both host
 * arrays are always given; a slot the rule does not use is left as it is).  step = the rule's 1-based count t. */
int smx_k_opt(int32_t rule, const float* hp, int32_t n_hp, int32_t n_tensors, const int32_t* sizes, float* params, const float* grads,
              float* m, float* v, int32_t step, float lr, float clipnorm, float* norms);
/* Clip + update by ANY of the launches that carry the optimiser's chunk body (smx_adam.h), over caller-given tensors laid out as smx_k_opt
 * lays them out (every tensor padded to 64 floats, 4096-float chunks).  hp[n_hp], sizes, params, grads, m, v as smx_k_opt's, none updated in place.
 * ip (int32): rule, n_tensors, carrier (smx_opt_carrier), wgs (sweep, sharded chain: persistent workgroups), world (sharded chain), use_sq,
 *   step (the 1-based count of optimiser steps, this one included), t0 (the step index at which the rule's state began: the rule's count is
 *   t = step - t0, and 1 while step <= t0), tied_t0, tied_t1 (tensor indices or -1), n_slots (length of sq_slots).
 * fp (float): lr, clipnorm (0: off), grad_scale, tied_inv.
 * use_sq = 0: the norms come from per-chunk partial sums made by the carrier's own norm pass.  use_sq != 0 (not the sharded chain): tensor i
 *   takes its sum of squares from sq_slots[sq_first[i] .. + sq_count[i]) if sq_count[i] > 0, else from a sweep of its own gradient.
 * SMX_CARRIER_SHARD runs the data-parallel chain of flag opt_shard on one device: the buffer cut into `world` equal slices at 64-float
 *   boundaries (through chunks where they fall); the slice-wise sums of squares once per rank into that rank's own partial array; the arrays
 *   summed in float32 in rank order (0 + rank 0 + rank 1 + ...); the norms; the update once per rank on its slice.
 * Out: params_out, m_out, v_out: the WHOLE padded buffers (sum of the padded sizes); norms [n_tensors] and *lr_t (the device's step size, read
 *   back from the step state) may be NULL.  Every device buffer lies between two guard bands of 0xFF bytes: *guards_ok = 1 if no band word
 *   changed.  A slot the rule does not use is 0xFF bytes before the launch instead of the caller's values: *unused_ok = 1 if it came back so. */
typedef enum { SMX_CARRIER_LAUNCH = 0, SMX_CARRIER_SWEEP = 1, SMX_CARRIER_SHARD = 2, SMX_CARRIER_BODY512 = 3 } smx_opt_carrier;
int smx_k_opt_carrier(const int32_t* ip, const float* fp, const float* hp, int32_t n_hp, const int32_t* sizes, const float* params,
                      const float* grads, const float* m, const float* v, const int32_t* sq_first, const int32_t* sq_count, const float* sq_slots,
                      float* params_out, float* m_out, float* v_out, float* norms, float* lr_t, int32_t* guards_ok, int32_t* unused_ok);
/* C[M,N] = op(A) * op(B) in fp32 on the MFMA path; transA: A given as [K,M];
 * transB: B given as [N,K]; split_k >= 1 (slabs summed on return).  tile_cfg 0: the library's choice of LDS tile; 100: the
 * direct bf16 x 3 form for deep contractions (transA = 0, K >= 512); 101 / 102: the minibatch-contracted weight-gradient forms
 * (transA = 1, transB = 0; 32 x 32 tiles / the gene-tile-owner panel form, N <= 128); 103: the gene-axis contraction of wide
 * panels (transA = 0, either layout of B, K >= 4096 after padding to 32, split_k = 1: one workgroup per K slice + the reduce
 * launch, plain float32 rows) -- test entries for those kernels. */
int smx_k_gemm(int transA, int transB, const float* A, const float* B, int32_t M, int32_t N, int32_t K,
               int32_t split_k, int32_t tile_cfg, float* C);
/* The whole output head of a training step at a wide gene panel in ONE launch (smx_headfused.hip; rows a-9, a-10 / a-11 and the head's
 * part of a-16): P = d W + bias (never stored) -> count log-likelihood of x and dP = grad_scale * d llk / d P (never stored) -> dW = d^T dP,
 * db = colsum(dP), dd = dP W^T.  Host arrays: x [B][G] counts (u16 != 0: through the uint16 store), d [B][128], W [128][k][G], bias [k][G]
 * (k = 2 NB / NBD, 3 ZINB / ZINBD); B <= 128, G >= 4096 after padding to 32.  Out: llk [B], dW [128][k][G],
 * db [k][G], dd [B][128], sumsq = sum of squares of dW (may be NULL); us (may be NULL): average device time of `reps` launches. */
int smx_k_head_fused(int likelihood, int u16, const float* x, const float* d, const float* W, const float* bias, int32_t B, int32_t G,
                     float grad_scale, int32_t reps, float* llk, float* dW, float* db, float* dd, float* sumsq, float* us);
/* The same launch `launches` (>= 2) times on the same inputs, every launch after the first compared on the device, bit for bit, with what
 * the first left (dW, db, the d d slabs, the likelihood partials): *n_differ = launches that differed, *first_word (may be NULL) = index of
 * the first differing word within [dW | db | slabs | partials] or -1.  Regression test of two hardware behaviours that made this kernel's
 * results timing-dependent (tools/isa_lint.py rules R1, R2). */
int smx_k_head_fused_stress(int likelihood, int u16, const float* x, const float* d, const float* W, const float* bias, int32_t B, int32_t G,
                            float grad_scale, int32_t launches, int32_t* n_differ, int64_t* first_word);
/* The kernels' noise function beside hiprand's own generator (BASELINE north_star: "sampling from a hiprand state per wavefront"): for
 * every counter quadruple (c0, c1, c2, c3) = (column block, cell id, step, stream | sample << 8) `ours` receives the four words the
 * kernels compute, `hiprand_words` the four words of ONE hiprand4() on a hiprandStatePhilox4_32_10_t set up by
 * hiprand_init(seed, subsequence = c2 | c3 << 32, offset = 4 * (c0 | c1 << 32)); c1 < 2^30 (the offset is 64 bits). */
int smx_k_hiprand(uint64_t seed, int32_t n, const uint32_t* counters, uint32_t* ours, uint32_t* hiprand_words);
/* Philox words / dropout multipliers / normals exactly as the kernels draw them. */
int smx_k_noise(uint64_t seed, int32_t stream, int32_t step, int32_t sample, const int64_t* cell_ids, int32_t B,
                int32_t width, float dropout_p, float* dropout_mult, float* normal);
/* The BatchNorm launches of a hidden layer by themselves (smx_bn.hip): split-K slab sum -> (bias | BatchNorm) -> activation -> dropout, and
 * its backward, over host arrays; the library's own dispatch picks the form (register-resident for 2 / 4 / 8 / 16 rows per thread, the
 * round trip above 1024 rows, the wide column-major form, the forms of activations other than ReLU).  No front, no riders.
 * ip (int32): S slabs, B rows, H columns, Hp (H padded to 8), ld (row stride of a slab, >= Hp), wide (slabs [S][Hp][128] column-major, B <= 128,
 * Hp <= 128; otherwise [S][B][ld]), batchnorm, training, update_moving, act (smx_activation), mask_ld, Philox stream, step, cell_base, world.
 * fp (float): momentum, eps, leak, drop_p.  gamma, beta, bias, the moving statistics: [Hp] (beyond H unread).  Dropout (training, drop_p > 0):
 * `mask` [B][mask_ld] holds the multipliers, or (mask NULL) they are drawn from Philox under (seed, stream, step) for cell cell_base + rows[b]
 * (rows NULL: b).  world > 0: SyncBatchNorm of `world` simulated ranks with B / world rows each -- phase 0 per rank into its own gather
 * buffer, the buffers summed, phase 1 per rank (world = 1 included; 0: the ordinary launch).  Out: out, xhat [B][Hp]; inv_std, batch_mean,
 * batch_var, the moving statistics after the launch [Hp] (any may be NULL).  Every output buffer lies between two guard bands of a fixed
 * pattern and starts as NaN: *guards_ok = 1 if no band word changed. */
int smx_k_bn_fwd(const int32_t* ip, const float* fp, const float* pre, const float* gamma, const float* beta, const float* bias,
                 const float* moving_mean, const float* moving_var, const float* mask, const int32_t* rows, uint64_t seed, float* out,
                 float* xhat, float* inv_std, float* batch_mean, float* batch_var, float* moving_mean_out, float* moving_var_out,
                 int32_t* guards_ok);
/* ... and the backward launch on ITS inputs: the d out slabs (laid out as `pre` above), the forward's out, xhat [B][Hp], inv_std [Hp], gamma,
 * beta [Hp], the dropout source as above.  ip: S, B, H, Hp, ld, wide, batchnorm, training, act, mask_ld, stream, step, cell_base, world;
 * fp: leak, drop_p.  Out: dpre [B][Hp]; dgamma, dbeta [max(world, 1)][Hp] (under SyncBatchNorm each rank's share); dbias [Hp] (without
 * BatchNorm); *guards_ok as above. */
int smx_k_bn_bwd(const int32_t* ip, const float* fp, const float* dout, const float* out, const float* xhat, const float* inv_std,
                 const float* gamma, const float* beta, const float* mask, const int32_t* rows, uint64_t seed, float* dpre, float* dgamma,
                 float* dbeta, float* dbias, int32_t* guards_ok);
/* The scVI gene head's launches by themselves (smx_scvi.hip), over host arrays in a training step's own layout: raw / planes [B][ld], plane c
 * of a row at c * plane_stride, Gp columns of which G are live (a step has Gp = G rounded up to 32, plane_stride = Gp, ld = k Gp; k = 2 for
 * nbd, 3 for zinbd).  The library's own dispatch picks the instance by Gp.  Every output lies between guard bands and starts as NaN
 * (*guards_ok as smx_k_bn_fwd).  The entries refuse shapes that would take a kernel outside a buffer; alignment (ld, plane_stride, Gp
 * multiples of 4), the train form's limit Gp <= 20480 and its null outputs are refused by the launchers: SMX_ERR_INVALID, no fallback.
 * smx_k_scvi_head_train -- the row-local training launch.  ip (int32): B, G, Gp, plane_stride, ld, likelihood (SMX_LLK_NBD / _ZINBD), x_u16,
 * n_x, ldx, Kl, ldh, ldwl, n_lib, x_identity, ldl, Philox stream, step, cell_base.  fp: clip_library, grad_scale, kl_weight (what multiplies
 * the library KL's gradient).  x [n_x][ldx]: float counts, or (x_u16) uint16; hl [B][ldh]; Wl [Kl][ldwl] (columns mu, s); bl [2]; library
 * [n_lib][2] (prior mean, variance); rows [B] or NULL (cell b = row b): the library row, and with x_identity = 0 the row of x; eps_in [B]
 * the injected library noise, or NULL (drawn from Philox under seed, stream, step for cell cell_base + rows[b]).  Out, all of the kernel's:
 * draw [B][ld]; llk_part (without the count constant), l, sig, eps, kl, dl [B]; latl, dlatl [B][ldl].  A NULL output reaches the launcher
 * as NULL. */
int smx_k_scvi_head_train(const int32_t* ip, const float* fp, const float* raw, const void* x, const float* hl, const float* Wl, const float* bl,
                          const float* library, const int32_t* rows, const float* eps_in, uint64_t seed, float* draw, float* llk_part, float* l,
                          float* sig, float* eps, float* kl, float* latl, float* dlatl, float* dl, int32_t* guards_ok);
/* ... the separate forward (ip: B, G, Gp, plane_stride, ld, k; fp: clip_library): raw [B][ld], l [B] -> planes [B][ld] (rate, theta[, gate]),
 * rho_raw [B][Gp] (the softmax before its clip) ... */
int smx_k_scvi_head_fwd(const int32_t* ip, const float* fp, const float* raw, const float* l, float* planes, float* rho_raw, int32_t* guards_ok);
/* ... and the separate backward on ITS inputs: planes, dplanes [B][ld], rho_raw [B][Gp], l [B] -> draw [B][ld], dl [B]. */
int smx_k_scvi_head_bwd(const int32_t* ip, const float* fp, const float* planes, const float* dplanes, const float* rho_raw, const float* l,
                        float* draw, float* dl, int32_t* guards_ok);
/* The label heads' launch by itself (smx_loss.hip), over host arrays in a training step's layout; the library's own dispatch picks the kernel
 * (the 'mixtril' head has its own).  ip (int32): kind (smx_label_likelihood), C (mixture components), B, P (label dimension), Pp (P rounded
 * up to 32), ld (row stride of raw / draw, >= planes x Pp; planes: 1 onehot / bernoulli, 2 nb / nbd / normal, 3 zinb / zinbd, 3 C mixnb /
 * mixgauss, 4 C mixzinb, C (2 + P) mixtril), ldy, n_rows, observed, add, backward.  fp: grad_scale.  raw [B][ld]; Y [n_rows][ldy]; rows [B]
 * or NULL (cell b = row b): the row of Y and of mask; mask [n_rows] bytes or NULL (every cell unlabelled unless observed).  llk [B] and
 * draw [B][ld] are read AND written: they reach the device as the caller filled them (the accumulator that add = 1 adds to; any pattern that
 * tells a word the launch left alone from a written zero) between guard bands (*guards_ok as smx_k_bn_fwd).  Refused with SMX_ERR_INVALID:
 * P < 1, 'mixtril' outside 1..64 dimensions or 2..4 components, another mixture outside 1..4 components, Pp != round_up(P, 32), ld below
 * planes x Pp, a row index outside Y. */
int smx_k_label_loss(const int32_t* ip, const float* fp, const float* raw, const float* Y, const int32_t* rows, const uint8_t* mask, float* llk,
                     float* draw, int32_t* guards_ok);
/* The predictive sampler by itself on caller-given planes [k][rows][G] (host; k planes of `likelihood`, direct / count_only as
 * smx_k_count_llk / smx_predict_sample): out [n_k][rows][G], the draws of rows 0 .. rows - 1 of a call with one Monte-Carlo draw
 * (s = 0) under `seed`.  rows <= 65535. */
int smx_k_plane_sample(int likelihood, int direct, int count_only, const float* planes, int32_t rows, int32_t G, uint64_t seed,
                       int32_t n_k, float* out);
/* The row selection of smx_predict_impute by itself: the two middle order statistics (G - 1) / 2 and G / 2 of each of n_rows rows
 * [n_rows][ld] (host, ld >= G; what lies beyond G in a row is not read) -> lo, hi [n_rows].  Rows hold non-negative values or NaN (what
 * an absolute difference is); -0 counts as +0 and a NaN sorts above +inf, as np.partition orders them. */
int smx_k_row_select(const float* rows, int32_t n_rows, int32_t G, int32_t ld, float* lo, float* hi);
/* The column kernels of smx_predict_correlate by themselves, on host columns cols [n_cols][n_cells] (gene-major).  smx_k_col_rank2:
 * rank2 [n_cols][n_cells] = 2 x scipy.stats.rankdata(column, 'average') and the nonfinite flags [n_cols].  smx_k_col_correlate: the ranks,
 * then the sums, with the operands and outputs of smx_predict_correlate (n_sel = n_cols).  n_cells <= 2^20. */
int smx_k_col_rank2(const float* cols, int32_t n_cols, int64_t n_cells, int32_t* rank2, int32_t* nonfinite);
int smx_k_col_correlate(const float* cols, int32_t n_cols, int64_t n_cells, const int32_t* prot_rank2, const double* prot_unit, int32_t P,
                        int64_t* sp_Sa, int64_t* sp_Saa, int64_t* sp_Sab, double* pe_mean, double* pe_Sxx, double* pe_Sxy, int32_t* nonfinite);

/* ---- clustering scores of a latent space (smx_cluster.hip; model-free: smx_init only) ----------- */
/* The distance sums of sklearn.metrics.silhouette_samples (Euclidean) for host cells Z [n_cells][D] with classes labels [n_cells] in
 * 0 .. n_labels - 1: a[i] = (sum over j of i's class c of |z_i - z_j|) / (n_c - 1), 0 for a singleton class; b[i] = the smallest, over the
 * classes c' != c with n_c' > 0, of (sum over j in c' of |z_i - z_j|) / n_c' (+inf when no other class has a cell).  Differences, squares,
 * sums, square roots and the per-class accumulation are float64 in the direct form sqrt(sum_d (z_i[d] - z_j[d])^2); no float atomics: the
 * order of every sum is a function of (n_cells, D, labels) alone, so two calls give the same bits.  A NaN or an infinity in Z (an infinity
 * is read as NaN) gives NaN in the a / b of every cell whose sums it enters.  1 <= D <= 128, 2 <= n_labels <= 256, 1 <= n_cells < 2^31,
 * every label in range: anything else is SMX_ERR_INVALID before any device work.  Device memory: 8 x slices x n_labels x n_cells bytes of
 * partial sums, slices = max(1, min(32, 1024 / ceil(n_cells / 256))). */
int smx_cluster_silhouette(const float* Z, int64_t n_cells, int32_t D, const int32_t* labels, int32_t n_labels, double* a, double* b);
/* Lloyd's iterations of n_init restarts run together, restart r from the cells init_idx [n_init][K] as its initial centres.  Per iteration
 * and restart: every cell goes to the centre with the smallest sum_d (z[d] - c[d])^2 (float64 on float64 centres, ties to the lowest index;
 * a NaN distance is never the smallest), then each centre becomes the float64 mean of its members, summed in a fixed order; an EMPTY
 * CLUSTER KEEPS ITS PREVIOUS CENTRE.  A restart stops at the first assignment that changes no label, at max_iter assignments at the latest;
 * n_iter [n_init] counts its assignments, the confirming one included.  What is returned belongs to the LAST assignment: the labels, the
 * centres it measured against (on convergence these are also the means of the labels) and inertia [n_init] = the float64 sum of its
 * smallest squared distances, in a fixed order.  *best: the restart of lowest inertia, ties to the lowest index; labels_best [n_cells] and
 * centres_best [K][D] are its; labels_all [n_init][n_cells] (may be NULL): every restart's.  A restart's results do not depend on the others
 * of the call.  1 <= D <= 128, 2 <= K <= 256, K <= n_cells < 2^31, 1 <= n_init <= 4096, max_iter >= 1, every init_idx in 0 .. n_cells - 1:
 * anything else is SMX_ERR_INVALID before any device work.  Device memory: 12 x n_init x n_cells bytes. */
int smx_cluster_kmeans(const float* Z, int64_t n_cells, int32_t D, int32_t K, const int32_t* init_idx, int32_t n_init, int32_t max_iter,
                       int32_t* labels_best, double* centres_best, double* inertia, int32_t* n_iter, int32_t* best, int32_t* labels_all);

/* ---- 1-D Gaussian mixtures of ProbabilisticEmbedding (smx_gmm.hip; model-free: smx_init only) ----------- */
/* One mixture of K Gaussians per column of the host matrix X [n_cells][C] (non-negative), R restarts per column, all C x R jobs together.
 * The training set of a column is the reference's normalize(test_mode=False): with remove_zeros the positive cells in cell order plus ONE
 * sample 0 if any cell was zero (else every cell); with log_norm t = log1p((double)fl32(fl32(x / fl32(s + eps)) * 1e4)), s the float64 sum
 * of the column in cell order (col_sum [C]) and eps FLT_EPSILON, else t = x; float64 from there on.  Restart r of column c starts from the
 * raw values init_raw [C][R][K] (normalised the same way): every sample goes to the nearest seed (ties to the lowest index), and from these
 * one-hot responsibilities an M-step: nk = sum r + 10 DBL_EPSILON, mean = sum r t / nk, var = sum r t^2 / nk - mean^2 + reg_covar, w = nk /
 * n_train.  Then for it = 1 .. max_iter: the E-step (log-sum-exp; lb = the mean log-likelihood), the M-step, stop at the first |lb - lb_prev|
 * < tol (lb_prev = -inf at it = 1).  Nothing is special-cased: an empty component gets mean 0 and variance reg_covar.  lower_bound, n_iter,
 * converged [C][R]: the last lb, the E-steps taken, whether the stop rule fired.  best [C]: the restart of highest lower bound, ties to the
 * lowest index, NaN last; weights, means, variances [C][K] are its; n_train [C].  params_all [C][R][3][K] (may be NULL): every restart's
 * weights, means, variances.  stats [5] (may be NULL): launches, host round trips of the loop, ms between the loop's events (its launches),
 * ms of the loop, ms of the call.  Every sum has an order that is a function of n_cells alone (slices = min(64, ceil(n_cells / 4096)); no
 * float atomics), so two calls give the same bits and a job's results do not depend on the other jobs of the call.  1 <= C <= 4096,
 * 2 <= K <= 8, 1 <= R <= 64, K <= n_train of every column, 1 <= n_cells < 2^31, max_iter >= 1, tol > 0, reg_covar >= 0, no negative or
 * non-finite entry in X or init_raw: anything else is SMX_ERR_INVALID before any device work.  Device memory: 12 x n_cells x C bytes (X and
 * its normalised float64 copy) + 8 x C x R x (slices x (3 K + 1) + 5 K + 2) bytes. */
int smx_gmm1d_fit(const float* X, int64_t n_cells, int32_t C, int32_t K, const float* init_raw, int32_t R, int32_t max_iter, double tol,
                  double reg_covar, int32_t remove_zeros, int32_t log_norm, double* lower_bound, int32_t* n_iter, int32_t* converged,
                  int32_t* best, double* weights, double* means, double* variances, int64_t* n_train, double* col_sum, double* params_all,
                  double* stats);
/* The embeddings of X [n_cells][C] under fitted mixtures weights, means, variances [C][K].  Normalisation as above in test mode: no zero
 * removal, s the column sum of THIS matrix.  prob [n_cells][C]: the MEAN of the responsibilities of the components order[c][positive_component
 * .. K - 1], order [C][K] being the components by increasing mean; bin [n_cells][C]: 1 where t >= threshold[c] (the normalised scale), else
 * 0; score [n_cells][C] (may be NULL): the log-likelihood of the sample.  Limits on C, K, n_cells and X as above, 1 <= positive_component <
 * K, order a permutation per column, positive finite weights and variances, finite means, no NaN threshold: anything else is
 * SMX_ERR_INVALID before any device work.  Device memory: (16 or 24 with score) x n_cells x C bytes. */
int smx_gmm1d_predict(const float* X, int64_t n_cells, int32_t C, int32_t K, const double* weights, const double* means, const double* variances,
                      const int32_t* order, int32_t positive_component, const double* threshold, int32_t log_norm, double* prob, float* bin,
                      double* score);

/* ---- full-covariance Gaussian mixture of the clustering scores (smx_gmm_full.hip; model-free: smx_init only) ----------- */
/* scikit-learn's GaussianMixture(K, covariance_type='full') loop on the host cells Z [n_cells][D], run from R starting labelings
 * init_labels [R][n_cells] (each entry in 0 .. K - 1), all restarts together, float64 throughout.  Restart r: one-hot responsibilities from
 * init_labels[r], then an M-step: nk = sum_n r_nk + 10 DBL_EPSILON, w_k = nk / n_cells, mu_k = sum_n r_nk z_n / nk, S_k = sum_n r_nk (z_n -
 * mu_k)(z_n - mu_k)^T / nk + reg_covar I in the two-pass form (means first, then differences; the lower triangle, mirrored), L_k = chol(S_k),
 * Linv_k = L_k^-1, logdet_k = -sum_d log L_k[d][d].  Then for it = 1 .. max_iter: the E-step l_nk = log w_k + logdet_k - (D log(2 pi) +
 * |Linv_k (z_n - mu_k)|^2) / 2 (the difference before the triangular product), r_nk = exp(l_nk - lse_n) with the row maximum taken out, lb =
 * the mean of lse_n; the M-step; stop at the first |lb - lb_prev| < tol (lb_prev = -inf at it = 1).  lower_bound, n_iter, converged [R]: the
 * last lb, the E-steps taken, whether the stop rule fired (at max_iter without it: converged = 0 and the parameters of the last M-step).
 * A restart whose covariance meets a Cholesky pivot that is not a positive finite number stops there: status[r] = 1, lower_bound[r] = NaN, it
 * ranks last; SMX_ERR_INVALID is returned only when EVERY restart failed (lower_bound, n_iter, converged and status are filled even then).
 * *best: the restart of highest lower bound, ties to the lowest index.  weights [K], means [K][D], covariances [K][D][D], chol_inv [K][D][D]
 * (Linv_k: lower triangular, zeros above the diagonal -- the one thing the E-step reads) are its; labels [n_cells] = argmax_k l_nk of a final
 * E-step under them, ties to the lowest k.  params_all (may be NULL): per restart K weights, K D means, K D D covariances, [R][K + K D + K D
 * D].  Every sum has an order that is a function of n_cells alone (slices = min(64, ceil(n_cells / 1024)); no float atomics): two calls give
 * the same bits, and a restart's results do not depend on the others of the call.  1 <= D <= 64, 2 <= K <= 256, K <= n_cells < 2^31, 1 <= R
 * <= 8, max_iter >= 1, tol > 0, reg_covar >= 0, every init_labels entry in range, no non-finite entry in Z: anything else is SMX_ERR_INVALID
 * before any device work.  Device memory: 8 R K n_cells bytes of responsibilities + 4 n_cells D (Z) + 4 (R + 1) n_cells (labels) + 8 R K
 * slices (D (D + 1) / 2 + D + 1) of partial sums + 8 R K (2 D D + D + 2) of parameters. */
int smx_gmm_full_fit(const float* Z, int64_t n_cells, int32_t D, int32_t K, const int32_t* init_labels, int32_t R, int32_t max_iter, double tol,
                     double reg_covar, double* lower_bound, int32_t* n_iter, int32_t* converged, int32_t* status, int32_t* best,
                     double* weights, double* means, double* covariances, double* chol_inv, int32_t* labels, double* params_all);
/* The E-step above on Z [n_cells][D] under given parameters: labels [n_cells] = argmax_k l_nk (ties to the lowest k), resp [n_cells][K] (may
 * be NULL) the responsibilities, score [n_cells] (may be NULL) lse_n, the log-likelihood of the cell.  logdet_k = sum_d log chol_inv_k[d][d].
 * Limits on D, K, n_cells and Z as above; positive finite weights, finite means, a finite chol_inv with a positive diagonal (what lies above
 * the diagonal is not read): anything else is SMX_ERR_INVALID before any device work.  Device memory: (8 K + 4 D + 4 (+ 8 with score)) n_cells
 * bytes. */
int smx_gmm_full_predict(const float* Z, int64_t n_cells, int32_t D, int32_t K, const double* weights, const double* means, const double* chol_inv,
                         int32_t* labels, double* resp, double* score);

/* ---- count-matrix preprocessing (smx_prep.hip; model-free: smx_init only) ----------- */
/* Both entries take a host matrix of n_cells x n_genes in the rows convention (x, indptr, cols, vals; the top of this header; every CSR
 * column in 0 .. n_genes - 1) and stream it through the device in blocks of block_rows rows (0: the library's choice, about 64 MiB of
 * tile; a given value is rounded up to a multiple of 64 and capped at 1 GiB of tile; CSR blocks cross as CSR and are expanded on the
 * device).  They work on a VIEW of the matrix: the value of entry (r, g) is f(x[r][g] / row_div[r]) in float32 with the IEEE division --
 * row_div [n_cells] float32 (NULL: no division), func 0 the identity, 1 log1pf, 2 expm1f.  n_cells < 2^31, n_genes <= 2^20, a row
 * divisor finite and not 0: anything else is SMX_ERR_INVALID before any device work.
 *
 * smx_prep_stats: the statistics of the view.  cell_total [n_cells]: the float64 sum of the cell's values over the genes (with col_mask
 * [n_genes] uint8, may be NULL: over the genes whose mask is not 0); cell_n_genes [n_cells]: its values > 0.  gene_sum, gene_sumsq
 * [n_genes]: the float64 sums of the float32 values and of their (exact) squares over the cells; gene_n_cells [n_genes]: its values > 0;
 * gene_n_above [n_genes] (with row_thresh [n_cells] float32, no NaN; both or neither): the cells whose value > row_thresh[r].  Every sum
 * has an order that is a function of the global row and column ids alone (a cell: 64 lanes over the columns, then a fixed tree; a gene:
 * slices of 64 consecutive rows added in row order, the slices in order; no atomics), so the results are the same bits for every
 * block_rows, for dense and CSR input, from call to call, and for "the view of X" and "the identity view of what smx_prep_apply wrote for
 * X under that view": the view is evaluated by the same kernel in both.
 *
 * smx_prep_apply: the view written out as float32.  out_dense [n_cells][n_genes] (may be x itself): with mean and sd [n_genes] float32
 * (both or neither) the value is then (v - mean[g]) / sd[g], and with clip != 0 it is then min(., max_value) (a NaN stays).  out_vals
 * [nnz], aligned with vals: CSR input without mean / sd / clip only -- the structure is unchanged, only the stored values cross.  Exactly
 * one of out_dense and out_vals.  Device memory of either entry: the tile, the staged CSR block, and 24 bytes x (block_rows / 64) x
 * n_genes of partial sums. */
int smx_prep_stats(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                   int32_t block_rows, int32_t func, const float* row_div, const uint8_t* col_mask, const float* row_thresh,
                   double* cell_total, int32_t* cell_n_genes, double* gene_sum, double* gene_sumsq, int64_t* gene_n_cells,
                   int64_t* gene_n_above);
int smx_prep_apply(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                   int32_t block_rows, int32_t func, const float* row_div, const float* mean, const float* sd, int32_t clip,
                   float max_value, float* out_dense, float* out_vals);

/* ---- exact PCA of a count matrix (smx_pca.hip; model-free: smx_init only) ----------- */
/* Both entries take the host matrix in the forms of smx_prep_stats (dense x, or CSR with x = NULL) and stream it in blocks of block_rows
 * rows as there.  n_genes <= 8192 on this route (the covariance takes 8 n_genes^2 bytes), and the limits of smx_prep_stats: anything else
 * is SMX_ERR_INVALID before any device work.
 *
 * smx_pca_cov: mean [n_genes] = the float64 column sums / n_cells, the sums in the order of smx_prep_stats' gene_sum (slices of 64
 * consecutive rows added in row order, the slices in order).  cov [n_genes][n_genes] = sum_r (x_r - mean)^T (x_r - mean) / (n_cells - 1),
 * the two-pass form: the operands are the float64 differences (double)x - mean, the products and sums are float64 on the matrix pipe
 * (v_mfma_f64_16x16x4_f64).  An entry's sum runs over the global rows in order, four at a time, in one accumulator that is carried exactly
 * between blocks; no atomics.  The lower triangle is computed and mirrored, so cov is exactly symmetric, and mean and cov are the same
 * bits for every block_rows, for dense and CSR input, and from call to call.  A constant column has variance exactly 0.  n_cells >= 2.
 * Device memory: the tile and the staged CSR block, 24 bytes x (block_rows / 64) x n_genes of partial sums, and 8 x (n_genes rounded up
 * to 64)^2 bytes of accumulators.
 *
 * smx_pca_project: out [n_cells][n_components] float32 = (x - mean) . components^T for mean [n_genes] and components
 * [n_components][n_genes] float64 (finite), 1 <= n_components <= 128.  Differences, products and sums are float64 (the same pipe),
 * rounded once to float32.  The genes of a sum are taken in chunks of 16; within chunk t the steps s = 0 .. 3 add genes 16 t + 4 q + s,
 * q = 0 .. 3 in this order: a function of n_genes alone, so out is the same bits for every block_rows and for dense and CSR input.
 * Device memory: the tile and the staged CSR block, 8 x n_components x n_genes bytes of components, 4 x block_rows x n_components of
 * output. */
int smx_pca_cov(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                int32_t block_rows, double* mean, double* cov);
int smx_pca_project(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                    int32_t block_rows, const double* mean, const double* components, int32_t n_components, float* out);

/* ---- exact nearest neighbours and UMAP connectivities (smx_knn.hip; model-free: smx_init only) ----------- */
/* smx_knn: for every cell i of the host cells Z [n_cells][D] float32 the k OTHER cells j != i with the smallest d2(i, j) = sum_d (z_i[d] -
 * z_j[d])^2, float64 in the direct form (four chains by d mod 4 with fma, then (s0 + s1) + (s2 + s3); never the Gram form).  The candidates
 * are ordered by (d2, j) ascending, a total order: the result does not depend on how the library cuts the work (the j range is cut into
 * max(1, min(32, 1024 / ceil(n_cells / 256))) slices whose sorted lists a second launch merges; developer knob "knn_slices"), and
 * duplicated cells are ordinary neighbours at distance 0.  idx [n_cells][k] int32, dist [n_cells][k] float64 = sqrt(d2), nearest first.
 * No float atomics; two calls give the same bits.  1 <= D <= 128, 1 <= k <= 256, k < n_cells < 2^31, every entry of Z finite: anything
 * else is SMX_ERR_INVALID before any device work.  Device memory: 12 x slices x k x n_cells bytes of lists, 4 n_cells D (Z), 12 k
 * n_cells (results).  The cost is n_cells^2 x D float64 operations: exact by design, no approximate search is built.
 *
 * smx_knn_umap: UMAP's smooth_knn_dist and compute_membership_strengths (local_connectivity = 1, bandwidth = 1) on a neighbour table
 * idx / dist [n_cells][K] whose column 0 is the cell itself at distance 0 and whose other K - 1 columns are smx_knn's, float64, one thread
 * per row.  target = log2(K).  rho = the first strictly positive distance of the row in column order, 0 without one.  lo = 0, hi = inf,
 * mid = 1; at most 64 rounds: psum = the sum over columns 1 .. K - 1, in order, of exp(-(d - rho) / mid) where d - rho > 0 and of 1
 * otherwise; stop when |psum - target| < 1e-5; if psum > target then hi = mid, mid = (lo + hi) / 2, else lo = mid and mid = 2 mid while
 * hi is infinite, (lo + hi) / 2 after.  sigma = max(mid, floor), floor = 1e-3 x the mean of the row (column 0 included, summed in column
 * order) when rho > 0, else 1e-3 x the mean of the whole table (ONE fixed-order float64 reduction: 256 strided partials, the lanes of a
 * wave by halving, then the four waves).  weight [n_cells][K]: 0 where idx names the cell itself, 1 where d - rho <= 0 or sigma == 0,
 * else exp(-(d - rho) / sigma).  rho, sigma [n_cells].  2 <= K <= 257, 1 <= n_cells < 2^31, every idx in 0 .. n_cells - 1, every dist
 * finite and >= 0: anything else is SMX_ERR_INVALID before any device work.  Device memory: 28 K n_cells bytes. */
int smx_knn(const float* Z, int64_t n_cells, int32_t D, int32_t k, int32_t* idx, double* dist);
int smx_knn_umap(const int32_t* idx, const double* dist, int64_t n_cells, int32_t K, double* rho, double* sigma, double* weight);

/* ---- t-SNE embeddings (smx_tsne.hip; model-free: smx_init only) ----------- */
/* scikit-learn's TSNE(method='barnes_hut') objective with the tree replaced by the EXACT sum over all pairs (its angle -> 0 limit), all in
 * float64.  The joint P between smx_tsne_affinities and the other two entries is host work: A = the CSR of cond_p on the kNN support,
 * P = (A + A^T) / sum(A + A^T), columns sorted, explicit zeros kept out (sisua_amd/neighbors.py).
 *
 * smx_tsne_affinities: scikit-learn's _binary_search_perplexity on smx_knn's table idx / dist [n_cells][k] (the k OTHER cells; k =
 * min(n_cells - 1, floor(3 perplexity + 1)) is scikit-learn's support and the caller's business), one thread per row.  d2_j = dist_j x
 * dist_j.  beta = 1, beta_min = -inf, beta_max = +inf; at most 100 rounds: p_j = exp(-d2_j x beta), sum = the p_j added in column order,
 * a sum equal to 0 replaced by (double)1e-8f; p_j = p_j / sum; H = log(sum) + beta x (the d2_j x p_j added in column order); stop when
 * |H - log((double)(float)perplexity)| <= (double)1e-5f (both constants are float32 values in scikit-learn); if H is above the target
 * then beta_min = beta and beta = 2 beta while beta_max is infinite, (beta + beta_max) / 2 after; else beta_max = beta and beta = beta / 2
 * while beta_min is infinite, (beta + beta_min) / 2 after.  No row-minimum shift, as in scikit-learn: a row whose every exp underflows
 * keeps p = 0.  No operation is fused.  cond_p [n_cells][k] = the p_j of the last round run, beta [n_cells] = the beta they were formed
 * with.  1 <= k <= 256, 4 <= n_cells, k < n_cells < 2^31, 1 <= perplexity < n_cells, every idx in 0 .. n_cells - 1, every dist finite and
 * >= 0: anything else is SMX_ERR_INVALID before any device work.  Device memory: 16 k n_cells bytes.
 *
 * The problem of the other two entries: P as CSR (indptr [n_cells + 1], cols, p) with indptr[0] = 0, rows that do not shrink, columns in
 * 0 .. n_cells - 1 and strictly increasing within a row, every p finite and > 0; an embedding Y [n_cells][n_components] float64, finite;
 * 1 <= n_components <= 3; 4 <= n_cells < 2^31.  Anything else is SMX_ERR_INVALID before any device work.
 *   w_ij = 1 / (1 + |y_i - y_j|^2), the IEEE division, |.|^2 = d_0 d_0 then fma(d_c, d_c, .) for c = 1, 2;   Z = sum_{i != j} w_ij
 *   grad_i = 4 [ sum_{j in row i of P} (exaggeration p_ij) w_ij (y_i - y_j)  -  (1 / Z) sum_{j != i} w_ij^2 (y_i - y_j) ]
 *   KL = sum_{p_ij > 0} p_ij log((p_ij Z) / w_ij), always with the un-exaggerated p
 * The repulsive pass is an n-body sweep: the j range is cut into max(1, min(32, 1024 / ceil(n_cells / 256))) slices (a function of
 * n_cells alone; developer knob "tsne_slices"); a thread adds w and w^2 (y_i - y_j) over its slice in j order with fma, and the slices
 * are added in slice order.  Z, the KL and the squared gradient norm are each ONE fixed-order reduction over the cells (1024 strided
 * partials, the lanes of a wave by halving, the sixteen waves by halving).  The attractive sum of a row is taken by sixteen lanes: lane l
 * adds the row's entries l, l + 16, ... (in column order) with fma, and the lanes are added by halving (l + 8, l + 4, l + 2, l + 1).
 * No float atomics: two calls give the same bits.  Another slice count adds the repulsive sums in another order: the neighbour table
 * and P do not depend on any slice knob, the gradient and the embedding may differ in their last bits and, the descent being chaotic,
 * an embedding after many iterations may differ visibly.
 *
 * smx_tsne_gradient: one evaluation -> grad [n_cells][n_components], *kl, *Z.  exaggeration finite and > 0.
 *
 * smx_tsne_fit: scikit-learn's descent from Y0, with the kernels of smx_tsne_gradient; Y, update, gains and P stay on the device and
 * only two doubles per reporting iteration come back.  The elementwise part is _gradient_descent's, every operation rounded: inc =
 * update x grad < 0; gains + 0.2 where inc, else gains x 0.8; gains >= 0.01; grad = grad x gains; update = momentum x update -
 * learning_rate x grad; Y = Y + update.  No recentring.  Schedule: iterations 0 .. min(250, max_iter) - 1 with exaggeration =
 * early_exaggeration and momentum 0.5, the rest with exaggeration 1 and momentum 0.8; as scikit-learn's two calls do, each phase
 * starts from update = 0 and gains = 1.  Iteration i reports when (i + 1) % 50 == 0 or it is the last of its phase: kl_trace[i] = KL at
 * the embedding the iteration started from (every other entry of kl_trace [max_iter] is NaN).  Where (i + 1) % 50 == 0 the phase ends
 * early when the norm of the gains-scaled gradient is <= min_grad_norm, and the second phase also when the KL has not improved for more
 * than n_iter_without_progress iterations; as in scikit-learn an early end of the first phase starts the second at the next iteration.
 * *n_iter = the number of iterations run.  Y [n_cells][n_components]; update_out and gains_out (each may be NULL) the descent's other
 * state, same shape.  max_iter >= 1, early_exaggeration and learning_rate finite and > 0, min_grad_norm >= 0,
 * n_iter_without_progress >= 0.  The cost of an iteration is n_cells^2 pair evaluations (about 30 float64 operations with the division):
 * exact by design, no Barnes-Hut or FFT approximation is built.  Device memory: 8 x slices x (1 + n_components) x n_cells bytes of
 * partial sums, 32 n_components n_cells (Y twice, update, gains), P, 16 n_cells. */
int smx_tsne_affinities(const int32_t* idx, const double* dist, int64_t n_cells, int32_t k, double perplexity, double* cond_p, double* beta);
int smx_tsne_gradient(const int64_t* indptr, const int32_t* cols, const double* p, int64_t n_cells, int32_t n_components, const double* Y,
                      double exaggeration, double* grad, double* kl, double* Z);
int smx_tsne_fit(const int64_t* indptr, const int32_t* cols, const double* p, int64_t n_cells, int32_t n_components, const double* Y0,
                 int32_t max_iter, double early_exaggeration, double learning_rate, double min_grad_norm, int32_t n_iter_without_progress,
                 double* Y, double* kl_trace, int32_t* n_iter, double* update_out, double* gains_out);

/* ---- UMAP layout (smx_umap.hip; model-free: smx_init only) ----------- */
/* The layout optimisation of umap-learn's simplicial_set_embedding / optimize_layout_euclidean in its PER-EPOCH form (cuML's reproducible
 * mode): every force of an epoch is evaluated from the positions at the epoch's start and then applied, so the result does not depend
 * on the order in which threads run.  All float64; no operation is fused; int n -> double is exact.
 *
 * The problem: the prepared graph as CSR (indptr [n_cells + 1], cols, epochs_per_sample) -- host work in sisua_amd/neighbors.py: the
 * symmetric fuzzy graph with its entries below max / n_epochs dropped, e = max / w per stored entry, both directions of an edge stored.
 * indptr[0] = 0, rows that do not shrink, columns in 0 .. n_cells - 1, strictly increasing within a row and never the row itself, every e
 * finite and > 0, at most 2^31 - 1 entries; the graph is symmetric (the caller's business: the factor 2 below relies on it); Y0
 * [n_cells][n_components] finite; 1 <= n_components <= 3; 2 <= n_cells <= 2^31 - 1; 1 <= n_epochs <= 10000; 0 <= epoch_begin <=
 * epoch_end <= n_epochs; a, b, gamma finite and >= 0; initial_alpha finite; 0 <= negative_sample_rate <= 64; next_sample and
 * next_negative [entries] finite.  Anything else is SMX_ERR_INVALID before any device work.
 *
 * Schedule state of entry x (position in the CSR) with e = epochs_per_sample[x], S = negative_sample_rate, e_neg = e / S.  A run from
 * epoch 0 starts at next_sample = e, next_negative = e_neg (S = 0: next_negative = e; it is then never read or written).  In epoch n
 * (epoch_begin <= n < epoch_end) the entry is ACTIVE iff next_sample <= n.  An active entry draws m negatives,
 *   m = min(max(trunc((n - next_negative) / e_neg), 0), S x n_epochs)   (S = 0: m = 0)
 * (trunc: towards zero, umap-learn's (int); the clamp never acts on a state reached from the start above and bounds every other one),
 * then next_sample = next_sample + e and next_negative = next_negative + m x e_neg (the product rounded, then the sum).
 * alpha_n = initial_alpha x (1 - n / n_epochs).
 *
 * Forces on cell j in epoch n, all from Y as it stood when the epoch began: d = y_j - y_k per component, d2 = d_0 d_0 (+ d_1 d_1 (+ d_2 d_2))
 * added in component order, clip(x) = min(4, max(-4, x)), pb = pow(d2, b): ONE pow per pair, d2^(b-1) is formed as pb / d2.
 *   attraction of an active entry (j, k), when d2 > 0:   g = (((-2 a) b) (pb / d2)) / (a pb + 1);   term_c = 2 clip(g d_c)
 *     (the 2: the entry's own head term plus the tail term of the mirror entry (k, j), which has the same weight, hence the same
 *     schedule, and from the same positions is the same number);
 *   negative p = 0 .. m - 1 of that entry: r = word (p & 3) of philox4x32_10(x, n, p >> 2, 100; seed & 0xFFFFFFFF, seed >> 32) -- the Philox
 *     of every other kernel here, stream id 100 (ST_UMAP_NEG) -- and k = r % n_cells; skipped when d2 == 0 (k == j, or cells on top of each
 *     other: umap-learn >= 0.5 adds 0); otherwise   g = ((2 gamma) b) / ((0.001 + d2) (a pb + 1));   term_c = clip(g d_c).   Only j moves.
 *   y_j <- y_j + alpha_n x (the sum of the cell's terms).  A cell whose row is empty never moves.
 * The sum of a cell is taken by L lanes over the row in chunks of L entries: L = 16 for a row of at most 64 entries, L = 256 (a workgroup
 * of its own) for a longer one -- the hub of a kNN graph holds hundreds of entries.  Entry L c + l of the row belongs to lane l, which
 * alone reads and writes its two schedule doubles.  Per chunk, lane l first adds the attraction of its own entry, then the chunk's
 * negatives: they are numbered q = 0, 1, .. through the chunk's entries in row order (entry by entry, p ascending) and lane l adds the
 * negatives q = l, l + L, l + 2 L, ... in this order.  After the last chunk the lanes are added by halving: L = 16: l + 8, l + 4, l + 2,
 * l + 1; L = 256: within each wave of 64 lanes l + 32, l + 16, .. l + 1, then the four waves as (0 + 1) + (2 + 3).  The order
 * is a function of the row and its schedule alone: no float atomics, two calls give the same bits, and a run cut into pieces
 * (0 .. s, then s .. E with the schedule arrays and Y of the first piece) gives the bits of the whole.
 * One launch per epoch, Y in two copies (one read, one written, then swapped), no host round trip inside a call.  On return Y is the
 * embedding after epoch epoch_end - 1 and next_sample / next_negative (in/out) the schedule state at epoch_end.  Work: about entries x
 * (1 + negative_sample_rate) x n_epochs x mean(w / max) pair evaluations with one float64 pow each.  Device memory: 16 n_components
 * n_cells + 28 entries + 12 n_cells bytes.
 *
 * smx_umap_pow (tests): out[i] = the device's pow(x[i], b), the function the forces use; n >= 1, x finite and > 0, b finite. */
int smx_umap_layout(const int64_t* indptr, const int32_t* cols, const double* epochs_per_sample, int64_t n_cells, int32_t n_components,
                    const double* Y0, int32_t n_epochs, int32_t epoch_begin, int32_t epoch_end, double a, double b, double gamma,
                    double initial_alpha, int32_t negative_sample_rate, uint64_t seed, double* next_sample, double* next_negative, double* Y);
int smx_umap_pow(const double* x, double b, int64_t n, double* out);

/* ---- gene x protein mutual information (smx_mi.hip; model-free: smx_init only) ----------- */
/* scikit-learn's three kNN estimators per pair (gene column, protein column), float64, every distance the exact |a - b|.  The columns
 * arrive gene-major, prepared by the host (sisua_amd/mutual_info.py: a continuous column divided by its standard deviation and noised,
 * a discrete column as it is; labels compare by value, -0 as +0).  psi [n_cells + 1] and logn [n_cells + 1] are the host's tables
 * digamma(n) and log(n), n = 0 .. n_cells (entry 0 is never read): the device adds table entries and evaluates neither function.
 * k = n_neighbors, N = n_cells, nextafter(., 0) = the float64 just below.
 *   cc (both continuous; Kraskov et al., _compute_mi_cc):  d_ij = max(|x_i - x_j|, |y_i - y_j|);  r_i = nextafter(the k-th smallest d_ij
 *      over j != i, 0);  cx_i = #{j : |x_j - x_i| <= r_i} and cy_i alike, i itself counted (scikit-learn's nx + 1, ny + 1);
 *      mi = psi(N) + psi(k) - (sum psi(cx_i)) / N - (sum psi(cy_i)) / N.
 *   cd (continuous c, discrete d; Ross, _compute_mi_cd):  in a label group of count > 1, k_i = min(k, count - 1) and r_i = nextafter(the
 *      k_i-th smallest |c_j - c_i| over the OTHER cells of the group, 0); the cells whose label occurs once are dropped from everything;
 *      m_i = #{kept j : |c_j - c_i| <= r_i}, i among them; with n' kept cells mi = psi(n') + (sum psi(k_i)) / n' - (sum psi(count_i)) / n'
 *      - (sum psi(m_i)) / n', and 0 when no cell is kept.
 *   dd (both discrete; mutual_info_score):  over the non-empty cells of the contingency table in (gene label, protein label) order,
 *      the sum of (n_ab / N) (((logn[n_ab] - logn[n_a]) - logn[n_b]) + logn[N]).
 * Every value is clipped below at 0.  Two deviations from scikit-learn: its NearestNeighbors leaves the tree for the brute-force path in
 * label groups of 2 .. 2k + 1 cells, whose distances sqrt(x^2 + y^2 - 2xy) lose the host's 1e-10 noise -- here they stay exact; and where
 * no cell is kept scikit-learn raises.
 * Every column is sorted once (a stable radix sort of the cell indices on the order-preserving 64-bit pattern).  cc is an exact sweep over
 * the other cells, outward from the cell in the gene's sorted order, that stops where no cell further out can be among the k nearest: the
 * k-th smallest distance is a set function, so the result is that of the full sweep.  Every sum over the cells is ONE fixed-order
 * reduction, a function of n_cells alone (256 strided partials, the lanes of a wave by halving, the four waves); dd's terms are added
 * the same way over the positions of the runs.  No float atomics: the same bits from call to call and for every gene_chunk (the genes
 * sorted and held on the device at a time; 0: as many as 256 MB hold at 36 n_cells + 28 n_cells n_proteins bytes each).
 * 2 <= n_cells <= 2^20; n_genes, n_proteins >= 1 and n_genes x n_proteins < 2^31; 1 <= n_neighbors <= 8 (the sweep's register list) and n_neighbors < n_cells, as scikit-learn asks; every value
 * finite (SMX_ERR_INVALID names the first offending gene or protein column; checked on the device, before any estimator runs on the
 * chunk).  mi [n_genes][n_proteins].
 *
 * smx_k_mi_cells: ONE pair of columns -> the per-cell quantities, for tests.  cells [4][n_cells] int32 and radius [n_cells], indexed by
 * cell.  cc: planes 0, 1 = cx_i, cy_i; radius = r_i.  cd (either column discrete): plane 0 = k_i, 1 = count_i where kept else 0, 2 = m_i,
 * 3 = count_i of every cell; radius = r_i (0 where not kept).  dd: indexed by POSITION in (gene label, protein label) order: plane 2 =
 * n_ab at the first position of a run and 0 elsewhere, plane 3 = the cell at the position; planes 0 and 1 hold the terms as float64.
 * *mi = the pair's value. */
int smx_mutual_info(const double* xcols, const uint8_t* x_discrete, const double* ycols, const uint8_t* y_discrete, int64_t n_cells,
                    int32_t n_genes, int32_t n_proteins, int32_t n_neighbors, int32_t gene_chunk, const double* psi, const double* logn,
                    double* mi);
int smx_k_mi_cells(const double* x, int32_t x_discrete, const double* y, int32_t y_discrete, int64_t n_cells, int32_t n_neighbors,
                   const double* psi, const double* logn, int32_t* cells, double* radius, double* mi);

/* ---- ranking genes between groups of cells (smx_rankgroups.hip; model-free: smx_init only) ----------- */
/* What scanpy.tl.rank_genes_groups (the reference's SingleCellOMIC.rank_vars_groups) needs of size n_cells x n_genes; the closing formulas
 * are the host's (sisua_amd/rank_groups.py).  labels [n_cells] int32 in 0 .. n_groups - 1.
 *
 * smx_group_moments: the host matrix in the forms of smx_prep_stats (dense x, or CSR with x = NULL, streamed in blocks of block_rows rows
 * as there), twice.  count [n_groups]: the cells of every group.  sum, css [n_groups][n_genes] float64 and nnz [n_groups][n_genes] int64:
 * per group and gene the float64 sum of the float32 values, the sum of the squares of the float64 differences (double)x - mean with mean
 * = sum / count (the two-pass form, one FMA per term; 0 for an empty group), and the values != 0 (-0 is 0).  Every sum runs over the
 * group's GLOBAL rows in row order in one accumulator that is carried exactly between blocks; no atomics: the same bits for every
 * block_rows, for dense and CSR input, and from call to call.  A non-finite entry of x shows as a non-finite sum.  The limits of
 * smx_prep_stats, 1 <= n_groups <= 65535 and n_groups x (n_genes rounded up to 4) <= 2^26: anything else is SMX_ERR_INVALID before any
 * device work.  Device memory: the tile, the staged CSR block, and 24 bytes x n_groups x n_genes of accumulators.
 *
 * smx_group_ranksums: host columns cols [n_cols][n_cells] float32, gene-major (the layout of smx_k_col_rank2), finite.  reference = -1
 * (every group against the rest): the average ranks of a column over all n_cells cells (-0 ties with +0); rank2_sum [n_groups][n_cols] =
 * 2 x the sum of the ranks of the group's cells, tie_term [n_cols] = sum (t^3 - t) over the column's runs of t equal values.  reference
 * = a group: for every other group g the ranks are those within the cells of g and of the reference; rank2_sum [g] = 2 x the rank sum
 * of g's cells there and tie_term [n_groups][n_cols] row g = the tie sum of that comparison; the rows of the reference itself and of
 * an empty group are 0.  int64, exact: 1 <= n_cells <= 2^20 (2 n_cells^2 and n_cells^3 stay below 2^63), 1 <= n_groups <= 256: anything
 * else is SMX_ERR_INVALID before any device work.  One sort per column in either case (with a reference by (value, label),
 * and a prefix count of the reference's cells over the sorted order).  The columns are sorted and held on the device as many at a time
 * as 256 MB hold (16 n_cells bytes each, 28 n_cells with a reference); the integers do not depend on it. */
int smx_group_moments(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_cells, int32_t n_genes,
                      int32_t block_rows, const int32_t* labels, int32_t n_groups, int64_t* count, double* sum, double* css, int64_t* nnz);
int smx_group_ranksums(const float* cols, int32_t n_cols, int64_t n_cells, const int32_t* labels, int32_t n_groups, int32_t reference,
                       int64_t* rank2_sum, int64_t* tie_term);

/* ---- mini-batch k-means on the count matrix (smx_mbkmeans.hip; model-free: smx_init only) ----------- */
/* The matrix work of scikit-learn's MiniBatchKMeans.partial_fit / predict (the reference's SingleCellOMIC.clustering); the random draws,
 * the reassignment of starved centres and the bookkeeping are the host's (sisua_amd/minibatch_kmeans.py).  The host matrix comes in the
 * forms of smx_prep_stats: dense x [n_rows][n_genes] float32, or CSR with x = NULL.  centres [n_clusters][n_genes] float64.  Every squared
 * distance is the direct form sum_j ((double)x_j - c_j)^2 in float64, the columns added in an order that is a function of n_genes alone
 * (a zero of a CSR row adds its c_j^2 at its place): dense and CSR input give the same bits, and so do two calls.  The nearest centre:
 * ties go to the lowest index and a NaN distance is never the smallest (a row whose every distance is NaN or +inf: centre 0, distance
 * +inf).  No atomics.  Limits of all three: 2 <= n_clusters <= 256, 1 <= n_genes <= 32768, 1 <= n_rows < 2^31; anything else, a null
 * pointer or a malformed CSR is SMX_ERR_INVALID before any device work.
 *
 * smx_mbkmeans_seed: scikit-learn's _kmeans_plusplus with unit weights on one block of n_clusters <= n_rows <= 65536 rows (rows x
 * (n_genes rounded up to 4) <= 2^31: the block is held whole).  first: the first centre's row; u [n_clusters - 1][n_trials] float64 in
 * [0, 1), 1 <= n_trials <= 16: the draws of every further centre.  Per centre: the inclusive float64 scan of the rows' distances to their
 * closest centre; per trial the first row whose scan value is >= u x potential, the last row where there is none; the candidates'
 * distances to every row, min with the closest so far; every candidate's potential as a fixed-order sum; the lowest potential is kept
 * (ties to the lowest trial).  All n_clusters rounds run in stream order without a host round trip.  indices [n_clusters] int32: the
 * chosen rows; centres: those rows; potential [n_clusters]: the potential after each pick.  Device memory: the tile, the staged CSR
 * block, 8 x (n_trials + 1) x n_rows and 8 x (n_clusters + n_trials) x n_genes bytes.
 *
 * smx_mbkmeans_step: scikit-learn's _mini_batch_step without the reassignment, on one block (held whole, as above).  The block's labels
 * against `centres` (labels [n_rows] int32, or NULL) and *inertia, the fixed-order sum of the rows' smallest distances.  Then in place,
 * for every centre with m > 0 rows: centre = (centre x count + the sum of its rows in row order) / (count + m), each operation rounded
 * once, and count += m; a centre without rows is left alone.  counts [n_clusters] float64 in/out, finite and >= 0.  Device memory: the
 * tile, the staged CSR block, 12 x n_rows and 8 x n_clusters x n_genes bytes.
 *
 * smx_mbkmeans_predict: labels [n_rows] int32 and, where distance is not NULL, the smallest squared distance [n_rows] float64 of every
 * row.  The matrix is streamed in blocks of block_rows rows as in smx_prep_stats (0: the library's choice); no result depends on it.
 * Device memory: the tile, the staged CSR block, 12 x n_rows and 8 x n_clusters x n_genes bytes. */
int smx_mbkmeans_seed(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                      int32_t n_clusters, int32_t n_trials, int64_t first, const double* u, int32_t* indices, double* centres,
                      double* potential);
int smx_mbkmeans_step(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                      int32_t n_clusters, double* centres, double* counts, int32_t* labels, double* inertia);
int smx_mbkmeans_predict(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                         int32_t block_rows, int32_t n_clusters, const double* centres, int32_t* labels, double* distance);

/* ---- Louvain communities of a symmetric graph (smx_louvain.hip; model-free: smx_init only) ----------- */
/* The reference's SingleCellOMIC.louvain (scanpy.tl.louvain there) as a deterministic method: synchronous within the colour classes of a
 * fixed colouring, every sum an exact integer (tests/louvain_ref.py restates it in NumPy and the device reproduces
 * that label for label).  The graph: a CSR adjacency [n][n], indptr int64 [n + 1], cols int32, weights float64 or NULL (unit weights on
 * the stored support).  Weights are quantised once, q = llrint(w / max w x 2^30); entries of q == 0 are dropped; every degree, total and
 * internal weight is an int64 sum of q, so no result depends on the order of a row's columns, on the launch geometry or on the call.  A
 * diagonal entry counts once in its vertex's degree k_v and once in its community's internal weight; m2 = sum k_v; Q = sum_c (in_c / m2 -
 * resolution (tot_c / m2)^2), the communities' terms added in the halving order of the analysis kernels' fixed-order sums.
 * Limits: 1 <= n <= 2^24, at most 2^31 - 1 entries, weights finite and >= 0, no column twice in a row, symmetric support and values,
 * resolution and tol finite and >= 0, max_sweeps >= 1, max_levels >= 1: anything else is SMX_ERR_INVALID before any device work.
 *
 * smx_louvain: the whole multi-level loop.  A level colours its graph (greedy in decreasing (mix32(v), -v), self loops ignored), starts
 * from singletons and sweeps over the colours; the vertices of one colour decide from the state at the start of the colour's turn: gain(D)
 * = kin_D - (resolution k_v tot_D) / m2 for a neighbouring community, tot_own - k_v in place of tot_D for the own one, float64 with every
 * operation rounded once; a vertex moves to the best (ties to the lowest id) only if that is strictly better than staying.  A level
 * ends when a sweep moves nothing, gains at most tol in Q, or lowers Q (its labels are then put back), or after max_sweeps.  Communities
 * are numbered in order of their lowest member and become the next level's vertices; levels repeat until one merges nothing or max_levels
 * have run.  labels [n] int32: the final ids by decreasing size, ties to the lowest member.  *n_levels: the levels run, the last (which
 * merged nothing) included, 0 for a graph without weight (every vertex its own community).  Per level, arrays of max_levels entries:
 * modularity (Q at its end), level_size (its communities), sweeps, colours.  The graph crosses to the device once; the host reads back a
 * few scalars per pair of colouring rounds, per sweep and per level.  Device memory: about 64 bytes per entry and 180 per vertex.
 *
 * smx_louvain_modularity: *q = Q of any partition, labels [n] int32 in 0 .. n - 1, with the same quantised integers.
 *
 * smx_louvain_table_degree: rows of up to this many stored entries are moved by one wave with a hash table in LDS, longer ones by one
 * workgroup with a sort (the developer knob louvain_table_degree lowers it; no result depends on it).  Needs no device. */
int smx_louvain(const int64_t* indptr, const int32_t* cols, const double* weights, int64_t n, double resolution, double tol,
                int32_t max_sweeps, int32_t max_levels, int32_t* labels, int32_t* n_communities, int32_t* n_levels, double* modularity,
                int64_t* level_size, int32_t* sweeps, int32_t* colours);
int smx_louvain_modularity(const int64_t* indptr, const int32_t* cols, const double* weights, int64_t n, const int32_t* labels,
                           double resolution, double* q);
int32_t smx_louvain_table_degree(void);

/* ---- L2-penalised logistic regression on the count matrix (smx_logreg.hip; model-free: smx_init only) ----------- */
/* What the reference's rank_vars_groups(method='logreg') asks of scikit-learn's LogisticRegression, as a deterministic full-batch solve
 * (tests/logreg_ref.py restates it in NumPy).  The host matrix comes in the forms of smx_prep_stats and is held whole in
 * one device tile [n_rows rounded up to 64][ld] float32, ld = n_genes rounded up to 4, across all iterations.  labels [n_rows] int32 in
 * 0 .. n_classes - 1; a fit needs at least one row of every class, an evaluation does not.  The objective, scikit-learn's in its mean form:
 *   F(W, b) = (1/N) sum_i loss_i + ||W||^2 / (2 C N), the intercept unpenalised (fit_intercept = 0: b is taken as 0 and gb is 0)
 * form 0, multinomial, 3 <= n_classes <= 256: W [n_classes][n_genes], b [n_classes] float64, loss_i = logsumexp(z_i) - z_{i, y_i}.
 * form 1, binary, n_classes = 2: ONE logit row, W [1][n_genes], b [1], loss_i = softplus(z_i) - y_i z_i (what scikit-learn fits for two
 * classes; not the two-class softmax, whose penalty differs by a factor of two).  Below Kz is the number of logit rows.
 * Everything is float64 from the float32 matrix on, every sum has an order that is a function of the shape alone and there are no
 * atomics: dense and CSR input give the same bits, and so do two calls.  A logit: each of 64 lanes adds its columns 256 i + 4 l .. + 3 in
 * rising order by fma from 0, the lanes by halving, the intercept last.  The gradient g_kj = (1/N) sum_i r_ik x_ij + w_kj / (C N), r_ik =
 * p_ik - [y_i = k]: slices of 64 global row ids in row order, then the slices in order; g_b,k = (1/N) sum_i r_ik.
 * Limits: n_genes <= 32768, n_rows < 2^31, rows x ld <= 2^31; C finite and > 0; matrix values, weights and intercepts finite: anything
 * else, a null pointer, a label out of range, a fit with a class without a row or a malformed CSR is SMX_ERR_INVALID before any device work.
 * Device memory: the tile, the staged CSR, 8 x n_rows x (Kz rounded up to 4), 8 x (n_rows / 64) x Kz x ld for the slices' partials
 * and, for the fit, 27 vectors of 8 x Kz x ld bytes.
 *
 * smx_logreg_eval: *F, gW [Kz][n_genes] and gb [Kz] at the given (W, b): the two matrix launches and their two closing launches alone.
 *
 * smx_logreg_fit: L-BFGS with memory 10 from zero (W0 = b0 = NULL) or from (W0, b0), all vectors on the device.  Armijo backtracking,
 * F(theta + t d) <= F + 1e-4 t g.d: the first trial is t = 1, or 1 / max|g| on the first iteration; each failure halves t; at most 30
 * trials (then the solve ends unconverged).  Where a trial changes F by at most 2^-43 |F| -- the rounding of two evaluations -- the
 * Armijo test would decide on noise: the trial is then accepted if it lowers max|g|.  A pair with s.y <= 0 is skipped.  It stops when max(|gW|, |gb|) <= tol (tol finite and > 0)
 * or after max_iter >= 1 iterations.  Out: W, b, *F and *gmax at them, *n_iter, *n_eval (evaluations of F and g), *converged.  An
 * objective that is not finite at the start point is SMX_ERR_NAN.  The host reads two scalars per evaluation and up to 69 dot products
 * per iteration.
 *
 * smx_logreg_decision: logits [n_rows][Kz] float64 (z = x.w + b as above), the matrix streamed in blocks of block_rows rows as in
 * smx_prep_stats (0: the library's choice); no bit depends on it. */
int smx_logreg_eval(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                    const int32_t* labels, int32_t n_classes, int32_t form, double C, int32_t fit_intercept, const double* W, const double* b,
                    double* F, double* gW, double* gb);
int smx_logreg_fit(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                   const int32_t* labels, int32_t n_classes, int32_t form, double C, int32_t fit_intercept, double tol, int32_t max_iter,
                   const double* W0, const double* b0, double* W, double* b, double* F, double* gmax, int32_t* n_iter, int32_t* n_eval,
                   int32_t* converged);
int smx_logreg_decision(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                        int32_t block_rows, int32_t n_classes, int32_t form, const double* W, const double* b, double* logits);

/* ---- gradient-boosted classification trees on a histogram of the count matrix (smx_gbt.hip; model-free: smx_init only) ----------- */
/* What the reference's get_importance_matrix / cal_importance / cal_dci ask of scikit-learn's GradientBoostingClassifier (loss='log_loss',
 * criterion='friedman_mse', subsample=1.0, max_features=None, prior init, Newton leaf values, x <= threshold goes left), with four stated
 * deviations that make the result one answer whatever the order of the sums (tests/gbt_ref.py restates it in NumPy):
 *   bins        a column (float32) with at most 256 distinct values has a bin per value; a wider one is cut between the sorted positions
 *               p - 1 and p, p = floor(j N / 256), j = 1 .. 255, wherever the two values differ.  A threshold is the float32 midpoint
 *               a/2 + b/2 of the two values a cut lies between (a where that rounds to b): bin(x) <= b exactly where x <= thresholds[b].
 *   statistics  per stage and class, the residual y_k - p_k and the curvature p_k (1 - p_k) as rint(v 2^40) int64: every per-(node, bin)
 *               sum, every count and every per-leaf sum is an exact integer (integer LDS and global atomics; n_rows <= 2^20).
 *   split rule  a candidate leaves min(nL, nR) >= min_samples_leaf; its improvement SL SL / nL + SR SR / nR - S S / n is evaluated in
 *               float64 from the integers in that order, without contraction; the largest wins, ties go to the lowest feature, then the
 *               lowest bin.  A node is a leaf at max_depth, with n < min_samples_split, n < 2 min_samples_leaf or no improvement > 0.
 *   leaf value  scale * sum r / sum h, 0 where sum h is 0; scale = (K - 1) / K, 1 for two classes; learning_rate is applied when the
 *               value is added to the raw scores (float64).
 * A tree is M = 2^(max_depth + 1) - 1 slots in heap order (the children of slot t are 2 t + 1 and 2 t + 2): feature int32 (-1: a leaf or
 * an unreached slot), threshold float32, left / right int32 (-1 on a leaf), value float64 (leaves), n int32 (0: unreached), improvement
 * float64 in residual units (the integer improvement x 2^-80).  Two classes fit ONE tree per stage (Kz = 1: the class-1 logit), K >= 3
 * classes K trees (Kz = K).  Dense and CSR input give the same bits, and so do two calls and every pass_pairs.
 * Limits: n_rows <= 2^20, n_genes <= 32768, rows x ld <= 2^31 (the float32 matrix is held whole while it is binned), 2 .. 32 classes,
 * max_depth 1 .. 6, learning_rate finite and > 0, min_samples_split >= 2, min_samples_leaf >= 1, every entry finite, every class with a
 * row: anything else is SMX_ERR_INVALID before any device work.
 *
 * smx_gbt_bin: thresholds [n_genes][255] float32 (zero behind the column's count), n_thresholds [n_genes], bins [n_genes][n_rows] uint8.
 * One workgroup per column sorts it (four 8-bit passes).
 *
 * smx_gbt_grow: the n_trees trees of one stage from given statistics q_r, q_h [n_trees][n_rows] int64 (|q_r| <= 2^41, 0 <= q_h <= 2^41)
 * over a bin matrix in smx_gbt_bin's layout; four launches per level, nothing read back in between.  leaf [n_trees][n_rows]: each cell's
 * leaf slot.  pass_pairs: the (class, node) pairs whose histograms one workgroup of the sweep holds in LDS, 1 .. 16 (0: 16 = 48 KiB); it
 * changes no bit.
 *
 * smx_gbt_fit: the stage loop.  init [Kz]: the raw scores of the prior.  n_iter_no_change > 0: scikit-learn's early stopping on the
 * validation rows (xv .. labels_val, the forms of x; they take no part in the bins or the trees): stage i is the last when its
 * validation loss + tol is below none of the last n_iter_no_change ones.  Out: the tree arrays [n_estimators][Kz][M] (stages behind
 * *n_estimators_out stay unreached), train_score / val_score [n_estimators]: the mean loss after each stage (x 2 for two classes, as
 * scikit-learn reports it).  The host reads two scalars per stage.
 *
 * smx_gbt_decision: raw [n_rows][n_outputs] float64 = init, then stage by stage + learning_rate * the row's leaf value, by x <=
 * threshold on the float32 entries; the matrix streamed in blocks of block_rows rows (0: the library's choice; no bit depends on it). */
int smx_gbt_bin(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                float* thresholds, int32_t* n_thresholds, uint8_t* bins);
int smx_gbt_grow(const uint8_t* bins, const int32_t* n_thresholds, const float* thresholds, const int64_t* q_r, const int64_t* q_h,
                 int64_t n_rows, int32_t n_genes, int32_t n_trees, int32_t max_depth, int64_t min_samples_split, int64_t min_samples_leaf,
                 double scale, int32_t pass_pairs, int32_t* feature, float* threshold, int32_t* left, int32_t* right, double* value,
                 int32_t* n, double* improvement, int32_t* leaf);
int smx_gbt_fit(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                const int32_t* labels, int32_t n_classes, const float* xv, const int64_t* v_indptr, const int32_t* v_cols, const float* v_vals,
                int64_t n_val, const int32_t* labels_val, int32_t n_estimators, double learning_rate, int32_t max_depth,
                int64_t min_samples_split, int64_t min_samples_leaf, int32_t n_iter_no_change, double tol, int32_t pass_pairs,
                const double* init, int32_t* feature, float* threshold, int32_t* left, int32_t* right, double* value, int32_t* n,
                double* improvement, int32_t* n_estimators_out, double* train_score, double* val_score);
int smx_gbt_decision(const float* x, const int64_t* indptr, const int32_t* cols, const float* vals, int64_t n_rows, int32_t n_genes,
                     int32_t block_rows, int32_t n_stages, int32_t n_outputs, int32_t max_depth, const int32_t* feature, const float* threshold,
                     const int32_t* left, const int32_t* right, const double* value, const double* init, double learning_rate, double* raw);

/* ---- padding audit (test instrument; never on the path of a step) ----------- */
/* The layout's invariant, read back from the device: every feature axis is padded to 32 and every tensor to 64 floats, and what lies
 * outside a tensor's logical extent (rows >= its rows; within each chunk, columns >= the chunk's width) stays exactly zero.  Counts, over
 * every tensor of the manifest, the elements of [offset, offset + count) outside the logical extent whose bits & 0x7fffffff != 0 (NaN and
 * denormals count, -0 does not).  which 0..3 as smx_get_tensor (and its rule for sharded optimiser moments: refused until
 * smx_opt_gather).  which = 4: the work buffers of the LAST pass, rows < its (stacked) batch, columns >= the logical width -- every MLP
 * layer's output (encoder, library encoder, decoder, discriminator), the latent draw z, scvi's library-latent head [B][32] (2 columns
 * in use), the gene head's gradient planes dP at columns >= n_genes of every plane, and what the last stacked evaluation decoder
 * (smx_marginal_llk, smx_score_llk, smx_predict) left of its last two layers (row-major, k-major or bf16-split form).
 * *n_bad: the count; first_tensor / first_offset / first_name (each may be NULL): the first offender -- its tensor index, the offset
 * inside it, its name.  which = 4: the index counts the buffers in the order above, whose number depends on the model (layers, planes,
 * scvi) -- identify a work buffer by first_name ("enc0 out", "z", "dP plane 1", "stacked dec0 (k-major)", ...).  Synchronises the model's stream; the buffer is walked on the host. */
int smx_pad_audit(smx_model* m, int32_t which, int64_t* n_bad, int32_t* first_tensor, int64_t* first_offset, char* first_name,
                  int32_t name_cap);
/* Writes `value` into the FIRST padded element of tensor `index` of buffer which = 0..3 (SMX_ERR_INVALID when the tensor has no padding):
 * exists so that a test can show that smx_pad_audit sees a violation.  which = 2 / 3 of a head's tensor: smx_get_tensor's rule for sharded
 * moments (refused until smx_opt_gather). */
int smx_pad_poke(smx_model* m, int32_t which, int32_t index, float value);

#ifdef __cplusplus
}
#endif
#endif /* SISUA_HIP_H_ */
