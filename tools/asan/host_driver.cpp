// host_driver.cpp -- the HOST-ONLY entry points of libsisua_hip.so under AddressSanitizer + UBSan ("Race detection /
// sanitizers").  Built and run by tools/asan_build.sh on the CPU: the library's translation units are compiled with
// `hipcc --cuda-host-only -fsanitize=address,undefined` (no device code, no GPU needed) and this program walks what can run without a device:
// the ABI queries, smx_shuffle_order, every argument / configuration check of smx_model_create up to its first device call, and the error paths
// of the accessors on a null model.  Any sanitizer report aborts with a non-zero status; "HOST DRIVER OK" is printed last.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/sisua_hip.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, smx_last_error()); ++failures; } } while (0)

static smx_config good_config() {
  smx_config c;
  memset(&c, 0, sizeof(c));
  c.abi_version = SMX_ABI_VERSION; c.model = SMX_MODEL_VAE; c.likelihood = SMX_LLK_ZINB; c.n_genes = 200; c.latent_dim = 10;
  c.n_enc = 2; c.enc_units[0] = 64; c.enc_units[1] = 32; c.n_dec = 1; c.dec_units[0] = 48;
  c.batchnorm = 1; c.log_norm = 1; c.dropout_enc = 0.1f; c.dropout_dec = 0.1f; c.beta = 1.f; c.alpha = 10.f; c.clip_library = 1e3f;
  c.bn_momentum = 0.99f; c.bn_eps = 1e-3f; c.lr = 1e-3f; c.adam_beta1 = 0.9f; c.adam_beta2 = 0.999f; c.adam_eps = 1e-7f; c.clipnorm = 100.f;
  c.max_batch = 64; c.seed = 8; c.n_components = 10; c.disc_units = 100; c.disc_layers = 2; c.gamma = 6.f; c.disc_leak = 0.2f;
  return c;
}

// a call that must fail cleanly on a box without a device: a status other than SMX_OK and a message (SMX_ERR_INVALID would mean the
// arguments here never reached the staging)
#define NO_DEVICE(call) do { const int rc_ = (call); if (rc_ == SMX_OK || rc_ == SMX_ERR_INVALID || strlen(smx_last_error()) == 0) { \
    printf("FAILED line %d: %s gave %d (last error: %s)\n", __LINE__, #call, rc_, smx_last_error()); ++failures; } } while (0)

static void model_free_entries() {
  const int N = 6, G = 4;
  std::vector<float> x((size_t)N * G), ones(4096, 1.f), out(4096);
  for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((i * 7) % 5);   // non-negative counts, zeros among them
  std::vector<double> dout(4096);
  std::vector<int32_t> iout(4096);
  std::vector<int64_t> lout(4096);
  // -- the kernel probes
  NO_DEVICE(smx_k_count_llk(SMX_LLK_NB, 0, x.data(), ones.data(), N, G, out.data(), out.data() + 64));
  { const int32_t sizes[2] = {5, 70};
    std::vector<float> p(75, 0.5f), g(75, 0.1f), m(75, 0.f), v(75, 0.f);
    NO_DEVICE(smx_k_adam(2, sizes, p.data(), g.data(), m.data(), v.data(), 1, 1e-3f, 0.9f, 0.999f, 1e-7f, 1.f, out.data()));
    NO_DEVICE(smx_k_opt(SMX_OPT_ADAM, nullptr, 0, 2, sizes, p.data(), g.data(), m.data(), v.data(), 1, 1e-3f, 1.f, out.data()));
    // the carriers' entry: valid arguments reach the staging on every carrier; every refusal comes before any device work
    const float fp[4] = {1e-3f, 5.f, 1.f, 1.f}, slots[4] = {1.f, 2.f, 3.f, 4.f};
    const int32_t sq_first[2] = {0, 0}, sq_count[2] = {0, 4};
    float lr_t = 0.f; int32_t guards = 0, unused = 0;
    auto carrier = [&](std::vector<int32_t> ip, const float* hp, int n_hp, const int32_t* sz, const int32_t* first, const int32_t* count) {
      return smx_k_opt_carrier(ip.data(), fp, hp, n_hp, sz, p.data(), g.data(), m.data(), v.data(), first, count, slots, out.data(), out.data() + 256,
                               out.data() + 512, out.data() + 768, &lr_t, &guards, &unused);
    };
    // ip: rule, n_tensors, carrier, wgs, world, use_sq, step, t0, tied_t0, tied_t1, n_slots
    NO_DEVICE(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr));
    NO_DEVICE(carrier({SMX_OPT_RMSPROP, 2, SMX_CARRIER_SWEEP, 2, 0, 1, 4, 3, 0, 1, 4}, nullptr, 0, sizes, sq_first, sq_count));
    NO_DEVICE(carrier({SMX_OPT_ADAMAX, 2, SMX_CARRIER_SHARD, 2, 3, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr));
    NO_DEVICE(carrier({SMX_OPT_SGD, 2, SMX_CARRIER_BODY512, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr));
    const float eps0[3] = {0.9f, 0.999f, 0.f}, eps_denormal[3] = {0.9f, 0.999f, 1e-39f}, ada0[2] = {0.f, 0.f}, rms0[3] = {0.9f, 0.9f, 0.f};
    const int32_t empty[2] = {5, 0}, beyond[2] = {0, 5};
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, eps0, 3, sizes, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(carrier({SMX_OPT_ADAMAX, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, eps_denormal, 3, sizes, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(carrier({SMX_OPT_ADAGRAD, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, ada0, 2, sizes, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(carrier({SMX_OPT_RMSPROP, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, rms0, 3, sizes, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(smx_k_opt(SMX_OPT_ADAM, eps0, 3, 2, sizes, p.data(), g.data(), m.data(), v.data(), 1, 1e-3f, 1.f, out.data()) == SMX_ERR_INVALID);
    EXPECT(carrier({SMX_OPT_ADAM, 2, 4, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);                    // no such carrier
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_SWEEP, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);    // sweep without workgroups
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_SHARD, 2, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);    // world 0
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_SHARD, 2, 2, 1, 1, 0, -1, -1, 4}, nullptr, 0, sizes, sq_first, sq_count) == SMX_ERR_INVALID);  // sharded chain with use_sq
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 1, 1, 0, -1, -1, 4}, nullptr, 0, sizes, sq_first, beyond) == SMX_ERR_INVALID);   // slots past n_slots
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 1, 1, 0, -1, -1, 4}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);   // use_sq without tables
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 0, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);   // step 0
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, 2, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID);    // tied tensor 2 of 2
    EXPECT(carrier({SMX_OPT_ADAM, 2, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, empty, nullptr, nullptr) == SMX_ERR_INVALID);   // an empty tensor
    EXPECT(carrier({SMX_OPT_ADAM, 4096, SMX_CARRIER_LAUNCH, 0, 0, 0, 1, 0, -1, -1, 0}, nullptr, 0, sizes, nullptr, nullptr) == SMX_ERR_INVALID); }
  NO_DEVICE(smx_k_gemm(0, 0, ones.data(), ones.data(), 8, 8, 8, 1, 0, out.data()));
  { const int B = 2, Gh = 4096;   // (the fused head's smallest panel)
    std::vector<float> xh((size_t)B * Gh, 1.f), d((size_t)B * 128, 0.1f), W((size_t)128 * 2 * Gh, 0.01f), bias((size_t)2 * Gh, 0.f), dW(W.size()), db(bias.size());
    int32_t n_differ = 0; int64_t first = 0;
    NO_DEVICE(smx_k_head_fused(SMX_LLK_NB, 1, xh.data(), d.data(), W.data(), bias.data(), B, Gh, 1.f, 0, out.data(), dW.data(), db.data(), out.data() + 64, nullptr, nullptr));
    NO_DEVICE(smx_k_head_fused_stress(SMX_LLK_NB, 0, xh.data(), d.data(), W.data(), bias.data(), B, Gh, 1.f, 2, &n_differ, &first)); }
  { const uint32_t counters[8] = {0, 1, 2, 3, 4, 5, 6, 7}; uint32_t ours[8], theirs[8];
    NO_DEVICE(smx_k_hiprand(8, 2, counters, ours, theirs)); }
  { const int64_t ids[3] = {0, 5, 9};
    NO_DEVICE(smx_k_noise(8, 1, 0, 0, ids, 3, 8, 0.1f, out.data(), out.data() + 64)); }
  { const int32_t fwd[15] = {1, 4, 8, 8, 8, 0, 1, 1, 1, SMX_ACT_RELU, 0, 0, 0, 0, 0}, bwd[14] = {1, 4, 8, 8, 8, 0, 1, 1, SMX_ACT_RELU, 0, 0, 0, 0, 0};
    const float ffp[4] = {0.99f, 1e-3f, 0.f, 0.f}, bfp[2] = {0.f, 0.f};
    int32_t guards = 0;
    NO_DEVICE(smx_k_bn_fwd(fwd, ffp, ones.data(), ones.data(), ones.data(), nullptr, ones.data(), ones.data(), nullptr, nullptr, 8, out.data(), out.data() + 64,
                           nullptr, nullptr, nullptr, nullptr, nullptr, &guards));
    NO_DEVICE(smx_k_bn_bwd(bwd, bfp, ones.data(), ones.data(), ones.data(), ones.data(), ones.data(), ones.data(), nullptr, nullptr, 8, out.data(), out.data() + 64,
                           out.data() + 128, nullptr, &guards)); }
  { // the scVI head's entries: B 2, G 5, Gp 32, k 3 (ld 96); a row id beyond the library and a stride short of the planes are refused before staging
    const int32_t tr[18] = {2, 5, 32, 32, 96, SMX_LLK_ZINBD, 0, 2, 32, 3, 3, 2, 2, 0, 4, 65, 0, 0}, sep[6] = {2, 5, 32, 32, 96, 3}, rows_bad[2] = {0, 2};
    const float tfp[3] = {1e3f, -0.5f, 0.1f};
    int32_t guards = 0;
    float* o = out.data();
    auto train = [&](const int32_t* ip, const int32_t* rows, float* draw) {
      return smx_k_scvi_head_train(ip, tfp, ones.data(), ones.data(), ones.data(), ones.data(), ones.data(), ones.data(), rows, nullptr, 8, draw, o + 256, o + 300,
                                   o + 310, o + 320, o + 330, o + 340, o + 360, o + 380, &guards);
    };
    NO_DEVICE(train(tr, nullptr, o));
    EXPECT(train(tr, rows_bad, o) == SMX_ERR_INVALID);
    { int32_t bad[18]; memcpy(bad, tr, sizeof(bad)); bad[4] = 64; EXPECT(train(bad, nullptr, o) == SMX_ERR_INVALID); }
    { int32_t bad[18]; memcpy(bad, tr, sizeof(bad)); bad[5] = SMX_LLK_NB; EXPECT(train(bad, nullptr, o) == SMX_ERR_INVALID); }
    NO_DEVICE(smx_k_scvi_head_fwd(sep, tfp, ones.data(), ones.data(), o, o + 256, &guards));
    EXPECT(smx_k_scvi_head_fwd(sep, tfp, ones.data(), ones.data(), nullptr, o + 256, &guards) == SMX_ERR_INVALID);
    NO_DEVICE(smx_k_scvi_head_bwd(sep, tfp, ones.data(), ones.data(), ones.data(), ones.data(), o, o + 256, &guards));
    EXPECT(smx_k_scvi_head_bwd(sep, tfp, ones.data(), ones.data(), ones.data(), ones.data(), o, nullptr, &guards) == SMX_ERR_INVALID); }
  NO_DEVICE(smx_k_plane_sample(SMX_LLK_NB, 0, 1, ones.data(), N, G, 8, 1, out.data()));
  NO_DEVICE(smx_k_row_select(x.data(), N, G, G, out.data(), out.data() + 64));
  // -- correlation: G columns of N cells, one protein column
  { std::vector<int32_t> prank(N); std::vector<double> punit(N, 0.25);
    for (int i = 0; i < N; ++i) prank[i] = 2 * (i + 1);
    NO_DEVICE(smx_k_col_rank2(x.data(), G, N, iout.data(), iout.data() + 64));
    NO_DEVICE(smx_k_col_correlate(x.data(), G, N, prank.data(), punit.data(), 1, lout.data(), lout.data() + 64, lout.data() + 128, dout.data(), dout.data() + 64,
                                  dout.data() + 128, iout.data())); }
  // -- clustering and the mixtures: N cells, 2 classes / components
  { const int32_t labels[N] = {0, 1, 0, 1, 0, 1}, init_idx[2] = {0, 1}, order[2 * G] = {0, 1, 0, 1, 0, 1, 0, 1};
    const float init_raw[2 * G] = {0.f, 3.f, 0.f, 3.f, 0.f, 3.f, 0.f, 3.f};
    const std::vector<double> half((size_t)2 * G, 0.5), thr(G, 1.0), chol = {1., 0., 0., 1., 1., 0., 0., 1.};
    NO_DEVICE(smx_cluster_silhouette(x.data(), N, 2, labels, 2, dout.data(), dout.data() + 64));
    NO_DEVICE(smx_cluster_kmeans(x.data(), N, 2, 2, init_idx, 1, 5, iout.data(), dout.data(), dout.data() + 64, iout.data() + 64, iout.data() + 128, nullptr));
    NO_DEVICE(smx_gmm1d_fit(x.data(), N, G, 2, init_raw, 1, 5, 1e-3, 1e-6, 0, 1, dout.data(), iout.data(), iout.data() + 64, iout.data() + 128, dout.data() + 64,
                            dout.data() + 128, dout.data() + 192, lout.data(), dout.data() + 256, nullptr, nullptr));
    NO_DEVICE(smx_gmm1d_predict(x.data(), N, G, 2, half.data(), half.data(), half.data(), order, 1, thr.data(), 1, dout.data(), out.data(), nullptr));
    NO_DEVICE(smx_gmm_full_fit(x.data(), N, 2, 2, labels, 1, 5, 1e-3, 1e-6, dout.data(), iout.data(), iout.data() + 64, iout.data() + 128, iout.data() + 192,
                               dout.data() + 64, dout.data() + 128, dout.data() + 192, dout.data() + 256, iout.data() + 256, nullptr));
    NO_DEVICE(smx_gmm_full_predict(x.data(), N, 2, 2, half.data(), half.data(), chol.data(), iout.data(), nullptr, nullptr)); }
  // -- preprocessing: the dense matrix, and the same entries as CSR
  { const int64_t indptr[N + 1] = {0, 1, 2, 2, 3, 4, 4};
    const int32_t cols[4] = {0, 3, 1, 2};
    const float vals[4] = {1.f, 2.f, 3.f, 4.f};
    NO_DEVICE(smx_prep_stats(x.data(), nullptr, nullptr, nullptr, N, G, 0, 1, ones.data(), nullptr, nullptr, dout.data(), iout.data(), dout.data() + 64,
                             dout.data() + 128, lout.data(), nullptr));
    NO_DEVICE(smx_prep_stats(nullptr, indptr, cols, vals, N, G, 0, 0, nullptr, nullptr, nullptr, dout.data(), iout.data(), dout.data() + 64, dout.data() + 128,
                             lout.data(), nullptr));
    NO_DEVICE(smx_prep_apply(x.data(), nullptr, nullptr, nullptr, N, G, 0, 1, ones.data(), nullptr, nullptr, 0, 0.f, out.data(), nullptr));
    NO_DEVICE(smx_prep_apply(nullptr, indptr, cols, vals, N, G, 0, 1, nullptr, nullptr, nullptr, 0, 0.f, nullptr, out.data()));
    // -- exact PCA on the same two forms: mean [G], two components [2][G]
    const std::vector<double> mean(G, 0.5), comp((size_t)2 * G, 0.25);
    NO_DEVICE(smx_pca_cov(x.data(), nullptr, nullptr, nullptr, N, G, 0, dout.data(), dout.data() + 64));
    NO_DEVICE(smx_pca_cov(nullptr, indptr, cols, vals, N, G, 0, dout.data(), dout.data() + 64));
    NO_DEVICE(smx_pca_project(x.data(), nullptr, nullptr, nullptr, N, G, 0, mean.data(), comp.data(), 2, out.data()));
    NO_DEVICE(smx_pca_project(nullptr, indptr, cols, vals, N, G, 0, mean.data(), comp.data(), 2, out.data()));
    // -- mini-batch k-means on the same two forms: 2 centres, 2 trials; each entry also refuses one argument set before any staging
    const double u[2] = {0.25, 0.75}, u_bad[2] = {0.25, 1.0};
    std::vector<double> cent((size_t)2 * G, 0.5), cnt(2, 0.0), cnt_bad = {1.0, -1.0};
    double inertia = 0.0;
    NO_DEVICE(smx_mbkmeans_seed(x.data(), nullptr, nullptr, nullptr, N, G, 2, 2, 1, u, iout.data(), dout.data(), dout.data() + 64));
    NO_DEVICE(smx_mbkmeans_seed(nullptr, indptr, cols, vals, N, G, 2, 2, 1, u, iout.data(), dout.data(), dout.data() + 64));
    EXPECT(smx_mbkmeans_seed(x.data(), nullptr, nullptr, nullptr, N, G, 2, 2, 1, u_bad, iout.data(), dout.data(), dout.data() + 64) == SMX_ERR_INVALID);
    EXPECT(smx_mbkmeans_seed(x.data(), nullptr, nullptr, nullptr, N, G, N + 1, 2, 1, u, iout.data(), dout.data(), dout.data() + 64) == SMX_ERR_INVALID);
    NO_DEVICE(smx_mbkmeans_step(x.data(), nullptr, nullptr, nullptr, N, G, 2, cent.data(), cnt.data(), iout.data(), &inertia));
    NO_DEVICE(smx_mbkmeans_step(nullptr, indptr, cols, vals, N, G, 2, cent.data(), cnt.data(), nullptr, &inertia));
    EXPECT(smx_mbkmeans_step(x.data(), nullptr, nullptr, nullptr, N, G, 2, cent.data(), cnt_bad.data(), iout.data(), &inertia) == SMX_ERR_INVALID);
    NO_DEVICE(smx_mbkmeans_predict(x.data(), nullptr, nullptr, nullptr, N, G, 0, 2, cent.data(), iout.data(), dout.data()));
    NO_DEVICE(smx_mbkmeans_predict(nullptr, indptr, cols, vals, N, G, 4, 2, cent.data(), iout.data(), nullptr));
    EXPECT(smx_mbkmeans_predict(x.data(), nullptr, nullptr, nullptr, N, G, 0, 257, cent.data(), iout.data(), nullptr) == SMX_ERR_INVALID);
    // -- logistic regression on the same two forms: three classes (multinomial) and two (binary, one logit row); every refusal -- a label out
    //    of range, a class without a row, C, tol, max_iter, a value that is not finite, a form that does not fit the classes -- before any staging
    const int32_t y3[N] = {0, 1, 2, 0, 1, 2}, y2[N] = {0, 1, 0, 1, 0, 1}, y_out[N] = {0, 1, 3, 0, 1, 2}, y_gap[N] = {0, 2, 2, 0, 2, 2};
    std::vector<double> W((size_t)3 * G, 0.1), b(3, 0.0), gW((size_t)3 * G), gb(3), W_nan = W;
    W_nan[5] = NAN;
    std::vector<float> x_inf = x;
    x_inf[7] = INFINITY;
    double F = 0.0, gmax = 0.0;
    int32_t n_iter = 0, n_eval = 0, conv = 0;
    auto eval = [&](const float* xd, const int32_t* y, int K, int form, double C, const double* w) {
      return smx_logreg_eval(xd, xd ? nullptr : indptr, xd ? nullptr : cols, xd ? nullptr : vals, N, G, y, K, form, C, 1, w, b.data(), &F, gW.data(), gb.data());
    };
    auto fit = [&](const float* xd, const int32_t* y, int K, int form, double C, double tol, int max_iter, const double* w0, const double* b0) {
      return smx_logreg_fit(xd, xd ? nullptr : indptr, xd ? nullptr : cols, xd ? nullptr : vals, N, G, y, K, form, C, 1, tol, max_iter, w0, b0, gW.data(),
                            gb.data(), &F, &gmax, &n_iter, &n_eval, &conv);
    };
    NO_DEVICE(eval(x.data(), y3, 3, 0, 1.0, W.data()));
    NO_DEVICE(eval(nullptr, y2, 2, 1, 0.5, W.data()));
    NO_DEVICE(fit(x.data(), y2, 2, 1, 1.0, 1e-4, 10, nullptr, nullptr));
    NO_DEVICE(fit(nullptr, y3, 3, 0, 1.0, 1e-4, 10, W.data(), b.data()));
    NO_DEVICE(smx_logreg_decision(x.data(), nullptr, nullptr, nullptr, N, G, 0, 3, 0, W.data(), b.data(), dout.data()));
    NO_DEVICE(smx_logreg_decision(nullptr, indptr, cols, vals, N, G, 4, 2, 1, W.data(), b.data(), dout.data()));
    EXPECT(eval(x.data(), y_out, 3, 0, 1.0, W.data()) == SMX_ERR_INVALID);
    NO_DEVICE(eval(x.data(), y_gap, 3, 0, 1.0, W.data()));                   // (an evaluation needs no row of every class; a fit does)
    EXPECT(fit(x.data(), y_gap, 3, 0, 1.0, 1e-4, 10, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(eval(x.data(), y3, 3, 0, 0.0, W.data()) == SMX_ERR_INVALID);
    EXPECT(eval(x.data(), y3, 3, 0, 1.0, W_nan.data()) == SMX_ERR_INVALID);
    EXPECT(eval(x.data(), y3, 3, 0, 1.0, nullptr) == SMX_ERR_INVALID);
    EXPECT(eval(x_inf.data(), y3, 3, 0, 1.0, W.data()) == SMX_ERR_INVALID);
    EXPECT(eval(x.data(), y3, 3, 1, 1.0, W.data()) == SMX_ERR_INVALID);      // the binary form with three classes
    EXPECT(eval(x.data(), y2, 2, 0, 1.0, W.data()) == SMX_ERR_INVALID);      // the multinomial form with two
    EXPECT(eval(x.data(), y3, 257, 0, 1.0, W.data()) == SMX_ERR_INVALID);
    EXPECT(fit(x.data(), y3, 3, 0, 1.0, 0.0, 10, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(fit(x.data(), y3, 3, 0, 1.0, NAN, 10, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(fit(x.data(), y3, 3, 0, 1.0, 1e-4, 0, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(fit(x.data(), y3, 3, 0, -1.0, 1e-4, 10, nullptr, nullptr) == SMX_ERR_INVALID);
    EXPECT(fit(x.data(), y3, 3, 0, 1.0, 1e-4, 10, W.data(), nullptr) == SMX_ERR_INVALID);   // half a warm start
    EXPECT(fit(x.data(), y3, 3, 0, 1.0, 1e-4, 10, W_nan.data(), b.data()) == SMX_ERR_INVALID);
    EXPECT(smx_logreg_decision(x.data(), nullptr, nullptr, nullptr, N, G, -1, 3, 0, W.data(), b.data(), dout.data()) == SMX_ERR_INVALID);
    EXPECT(smx_logreg_decision(x.data(), nullptr, nullptr, nullptr, N, G, 0, 3, 0, W.data(), b.data(), nullptr) == SMX_ERR_INVALID); }
  // -- neighbours: the N cells in G dimensions, 2 others each; then the table with the cell itself in front
  { std::vector<int32_t> tidx((size_t)N * 3);
    std::vector<double> tdist((size_t)N * 3);
    for (int i = 0; i < N; ++i) for (int c = 0; c < 3; ++c) { tidx[(size_t)i * 3 + c] = (i + c) % N; tdist[(size_t)i * 3 + c] = 0.5 * c; }
    NO_DEVICE(smx_knn(x.data(), N, G, 2, iout.data(), dout.data()));
    NO_DEVICE(smx_knn_umap(tidx.data(), tdist.data(), N, 3, dout.data(), dout.data() + 64, dout.data() + 128)); }
  // -- Louvain: a ring of the N vertices, columns out of order; the host's checks (two transposes) and the quantisation run before the device is
  //    asked for; a graph without weight needs no device at all
  { int64_t indptr[N + 1], lsize[4];
    int32_t cols[2 * N], labels[N], nc = 0, nl = 0, sweeps[4], colours[4];
    double w[2 * N], q[4], qq = 1.0;
    for (int i = 0; i <= N; ++i) indptr[i] = 2 * i;
    for (int i = 0; i < N; ++i) {
      cols[2 * i] = (i + 1) % N; cols[2 * i + 1] = (i + N - 1) % N;
      w[2 * i] = 1.0 + ((i + 1) % N == 0 ? 0 : i); w[2 * i + 1] = 1.0 + ((i + N - 1) % N == N - 1 ? 0 : i - 1);   // w(i, i + 1) = 1 + i, the closing edge 1
    }
    w[1] = 1.0;
    NO_DEVICE(smx_louvain(indptr, cols, nullptr, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours));
    NO_DEVICE(smx_louvain(indptr, cols, w, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours));
    NO_DEVICE(smx_louvain_modularity(indptr, cols, w, N, labels, 1.0, &qq));
    EXPECT(smx_louvain_table_degree() >= 64);
    { double bad[2 * N]; memcpy(bad, w, sizeof(bad)); bad[0] += 1.0;   // the values are not symmetric
      EXPECT(smx_louvain(indptr, cols, bad, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours) == SMX_ERR_INVALID); }
    { int32_t bad[2 * N]; memcpy(bad, cols, sizeof(bad)); bad[0] = 3;   // the support is not
      EXPECT(smx_louvain(indptr, bad, nullptr, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours) == SMX_ERR_INVALID); }
    { int32_t bad[2 * N]; memcpy(bad, cols, sizeof(bad)); bad[1] = bad[0];   // a column twice
      EXPECT(smx_louvain(indptr, bad, nullptr, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours) == SMX_ERR_INVALID); }
    EXPECT(smx_louvain(indptr, cols, nullptr, N, -1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours) == SMX_ERR_INVALID);
    { const double zero[2 * N] = {0.0};
      EXPECT(smx_louvain(indptr, cols, zero, N, 1.0, 1e-7, 10, 4, labels, &nc, &nl, q, lsize, sweeps, colours) == SMX_OK);
      EXPECT(nc == N && nl == 0 && labels[N - 1] == N - 1);
      EXPECT(smx_louvain_modularity(indptr, cols, zero, N, labels, 1.0, &qq) == SMX_OK && qq == 0.0); } }
}

int main() {
  EXPECT(smx_abi_version() == SMX_ABI_VERSION);
  EXPECT(smx_last_error() != nullptr);
  const int n_dev = smx_device_count();
  printf("devices visible: %d\n", n_dev);
  EXPECT(smx_init(-1) != SMX_OK);
  EXPECT(smx_init(n_dev + 5) != SMX_OK && strlen(smx_last_error()) > 0);

  // ---- smx_shuffle_order: the streaming shuffle of create_dataset (buffer larger / smaller than the data, empty data, bad picks)
  for (int n : {0, 1, 7, 1000, 3381}) for (int buffer : {1, 5, 1000, 5000}) {
    std::vector<int64_t> picks((size_t)n);
    std::vector<int32_t> out((size_t)n, -1);
    uint64_t s = 12345u + (uint64_t)n * 31u + (uint64_t)buffer;
    for (auto& p : picks) { s = s * 6364136223846793005ull + 1442695040888963407ull; p = (int64_t)(s >> 33); }
    EXPECT(smx_shuffle_order(n, buffer, picks.data(), out.data()) == SMX_OK);
    std::vector<char> seen((size_t)n, 0);
    for (int v : out) { EXPECT(v >= 0 && v < n && !seen[(size_t)v]); if (v >= 0 && v < n) seen[(size_t)v] = 1; }   // a permutation
  }
  { int64_t bad[3] = {1, -4, 2}; int32_t out[3]; EXPECT(smx_shuffle_order(3, 2, bad, out) != SMX_OK); }
  EXPECT(smx_shuffle_order(3, 0, nullptr, nullptr) != SMX_OK);
  EXPECT(smx_shuffle_order(-1, 4, nullptr, nullptr) != SMX_OK);

  // ---- smx_model_create: every check in front of the first device call
  smx_model* m = nullptr;
  smx_config c = good_config();
  EXPECT(smx_model_create(nullptr, &m) != SMX_OK && smx_model_create(&c, nullptr) != SMX_OK);
  auto refused = [&](const char* what, smx_config cfg) {
    smx_model* mm = nullptr;
    const int rc = smx_model_create(&cfg, &mm);
    if (rc == SMX_OK) { printf("NOT refused: %s\n", what); ++failures; smx_model_destroy(mm); }
    else if (rc != SMX_ERR_INVALID) { printf("%s: expected SMX_ERR_INVALID, got %d (%s)\n", what, rc, smx_last_error()); ++failures; }
  };
  { smx_config b = c; b.abi_version = SMX_ABI_VERSION - 1; refused("abi", b); }
  { smx_config b = c; b.n_genes = 0; refused("n_genes", b); }
  { smx_config b = c; b.latent_dim = -3; refused("latent_dim", b); }
  { smx_config b = c; b.max_batch = 0; refused("max_batch", b); }
  { smx_config b = c; b.n_enc = 0; refused("n_enc", b); }
  { smx_config b = c; b.n_dec = SMX_MAX_LAYERS + 1; refused("n_dec", b); }
  { smx_config b = c; b.model = 99; refused("model kind", b); }
  { smx_config b = c; b.likelihood = 17; refused("likelihood", b); }
  { smx_config b = c; b.n_labels = SMX_MAX_LABELS + 1; refused("n_labels", b); }
  { smx_config b = c; b.n_labels = 1; b.label_dim[0] = 5; b.label_llk[0] = SMX_LABEL_NB; refused("label heads on a VAE", b); }
  { smx_config b = c; b.n_labels = 2; b.label_dim[0] = 5; b.label_dim[1] = 4; b.label_observed[1] = 1; refused("observed head behind a label head", b); }
  // (an extra output on FVAE is built since round 5, several one-hot label variables behind it since round 6; what stays refused: more than 32
  // classes in all, a label head on the mixture-density posterior)
  { smx_config b = c; b.model = SMX_MODEL_FVAE; b.disc_layers = 2; b.disc_units = 8; b.n_labels = 3; b.label_dim[0] = 5; b.label_llk[0] = SMX_LABEL_NBD; b.label_observed[0] = 1;
    b.label_dim[1] = 20; b.label_llk[1] = SMX_LABEL_ONEHOT; b.label_dim[2] = 13; b.label_llk[2] = SMX_LABEL_ONEHOT; refused("33 classes of label variables on FVAE", b); }
  { smx_config b = c; b.model = SMX_MODEL_FVAE; b.disc_layers = 2; b.disc_units = 8; b.n_labels = 2; b.label_dim[0] = 3; b.label_llk[0] = SMX_LABEL_ONEHOT;
    b.label_dim[1] = 1; b.label_llk[1] = SMX_LABEL_ONEHOT; refused("a one-class label variable on FVAE", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCALE_POST; b.n_components = 3; b.n_labels = 1; b.label_dim[0] = 5; b.label_llk[0] = SMX_LABEL_NB; refused("label head on the mixture-density posterior", b); }
  { smx_config b = c; b.model = SMX_MODEL_FVAE; b.disc_layers = 0; refused("fvae discriminator depth", b); }
  { smx_config b = c; b.model = SMX_MODEL_FVAE; b.disc_leak = 1.5f; refused("fvae leak", b); }
  { smx_config b = c; b.model = SMX_MODEL_FVAE; b.n_labels = 1; b.label_llk[0] = SMX_LABEL_NB; b.label_dim[0] = 4; refused("fvae label kind", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCALE; b.n_components = 1; refused("scale components", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCALE_TRIL; b.latent_dim = 40; refused("scale tril latent width", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCALE_POST; b.n_components = 12; refused("scale posterior components", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCVI; b.likelihood = SMX_LLK_ZINB; b.n_encl = 1; b.encl_units[0] = 16; refused("scvi likelihood", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCVI; b.likelihood = SMX_LLK_ZINBD; b.n_encl = 0; refused("scvi library encoder", b); }
  { smx_config b = c; b.scvi_dispersion = 1; refused("dispersion option on a VAE", b); }
  { smx_config b = c; b.model = SMX_MODEL_SCVI; b.likelihood = SMX_LLK_ZINBD; b.n_encl = 1; b.encl_units[0] = 16; b.scvi_inflation = 7; refused("scvi inflation value", b); }
  { smx_config b = c; b.dropout_enc = 1.0f; refused("dropout rate", b); }
  { smx_config b = c; b.input_dropout = -0.1f; refused("input dropout rate", b); }
  // a VALID configuration: with a GPU the model is built and destroyed (every buffer through the sanitizer's allocator checks on the host side);
  // without one the first device call fails cleanly (SMX_ERR_HIP), nothing leaks, nothing is half-built
  {
    const int rc = smx_model_create(&c, &m);
    if (n_dev > 0) { EXPECT(rc == SMX_OK && m != nullptr); if (rc == SMX_OK) { EXPECT(smx_num_tensors(m) > 0); EXPECT(smx_model_destroy(m) == SMX_OK); } }
    else EXPECT(rc == SMX_ERR_HIP && strlen(smx_last_error()) > 0);
  }
  // ---- the model-free entry points, each once with valid, tiny arguments: without a device every one runs its host-side staging (argument
  // checks, gm_columns, the CSR checks, the optimiser's chunk table), fails at its first allocation and returns with nothing held
  if (n_dev == 0) model_free_entries();
  // ---- accessors on a null model
  EXPECT(smx_model_destroy(nullptr) == SMX_OK);
  EXPECT(smx_num_tensors(nullptr) == 0);
  { char name[8]; int32_t r, cc; EXPECT(smx_tensor_info(nullptr, 0, name, 8, &r, &cc) != SMX_OK); }
  EXPECT(smx_dataset_size(nullptr) <= 0);
  { int32_t st = 0; EXPECT(smx_get_step(nullptr, &st) != SMX_OK); }
  if (failures) { printf("HOST DRIVER: %d failure(s)\n", failures); return 1; }
  printf("HOST DRIVER OK\n");
  return 0;
}
