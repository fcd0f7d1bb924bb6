#include <atomic>
#include <cfloat>
// smx_model.hip -- model state: construction / destruction, tensors, BatchNorm statistics, noise injection, flags, timing.
#include "smx_model.h"

namespace smx {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error_cstr() { return g_err.c_str(); }

int add_tensor(smx_model* m, const std::string& name, int rows, int cols, int chunks, bool vec) {
  TensorInfo t;
  t.name = name; t.rows = vec ? 1 : rows; t.cols = cols; t.chunks = chunks;
  t.chunk_w = cols / chunks; t.chunk_wp = round_up(t.chunk_w, 32);
  t.rows_p = vec ? 1 : round_up(rows, 32);
  t.ld = chunks * t.chunk_wp;
  t.offset = m->flat_count;
  t.count = (size_t)t.rows_p * t.ld;
  m->flat_count += (t.count + 63) / 64 * 64;
  m->tensors.push_back(t);
  return (int)m->tensors.size() - 1;
}

int build_mlp(smx_model* m, std::vector<MlpLayer>& mlp, const char* prefix, int n_in, int n, const int32_t* units,
              int stream0, float drop_p, bool batchnorm, float leak) {
  for (int i = 0; i < n; ++i) {
    MlpLayer L;
    L.in = n_in; L.in_p = round_up(n_in, 32); L.out = units[i]; L.out_p = round_up(units[i], 32);
    std::string p = std::string(prefix) + std::to_string(i);
    L.tW = add_tensor(m, p + "/W", n_in, units[i], 1, false);
    if (batchnorm) {
      L.tGamma = add_tensor(m, p + "/gamma", 1, units[i], 1, true);
      L.tBeta = add_tensor(m, p + "/beta", 1, units[i], 1, true);
      L.bn = (int)m->bn_w.size();
      m->bn_w.push_back(units[i]); m->bn_wp.push_back(L.out_p);
    } else {
      L.tBias = add_tensor(m, p + "/b", 1, units[i], 1, true);
    }
    L.stream = stream0 + i; L.drop_p = drop_p; L.leak = leak;
    mlp.push_back(L);
    n_in = units[i];
  }
  return n_in;
}

// the sparse store's arrays (m->X aliases the expansion tile while it is in use)
void release_csr(smx_model* m) {
  if (!m->x_csr) return;
  if (m->csr_indptr) hipFree(m->csr_indptr);
  if (m->csr_cols) hipFree(m->csr_cols);
  if (m->csr_vals) hipFree(m->csr_vals);
  if (m->xbatch) hipFree(m->xbatch);
  m->csr_indptr = nullptr; m->csr_cols = nullptr; m->csr_vals = nullptr; m->xbatch = nullptr;
  m->X = nullptr; m->x_csr = false;
}
// the resident dataset: the sparse store (m->X aliased its expansion tile), the dense store and the side arrays
void release_dataset(smx_model* m) {
  auto fr = [](auto*& p) { if (p) hipFree(p); p = nullptr; };
  release_csr(m);
  fr(m->X); fr(m->library); fr(m->mask); fr(m->lgx1);
  for (int j = 0; j < SMX_MAX_LABELS; ++j) fr(m->Y[j]);
}

NoiseKey make_key(smx_model* m, int stream, int sample, bool training) {
  NoiseKey nk;
  nk.k0 = (uint32_t)(m->cfg.seed & 0xFFFFFFFFu);
  nk.k1 = (uint32_t)(m->cfg.seed >> 32);
  nk.step = 0;
  nk.stream = (uint32_t)((stream & 0xFF) | ((sample & 0xFFFFFF) << 8));
  nk.step_ptr = training ? &cur_state(m)->step : nullptr;
  nk.draw_rows = 0;
  return nk;
}

const Injected* inj(smx_model* m, int stream) {
  if (!m->use_injected) return nullptr;
  auto it = m->injected.find(stream);
  return it == m->injected.end() ? nullptr : &it->second;
}

void drop_graphs(smx_model* m) {  // captured graphs bake device pointers in: drop them when a buffer moves
  for (auto& kv : m->graphs) hipGraphExecDestroy(kv.second);
  m->graphs.clear();
}

// pack logical host tensor <-> padded internal layout
void pack(const TensorInfo& t, const float* host, std::vector<float>& dev) {
  dev.assign(t.count, 0.f);
  for (int r = 0; r < t.rows; ++r)
    for (int ch = 0; ch < t.chunks; ++ch)
      memcpy(&dev[(size_t)r * t.ld + (size_t)ch * t.chunk_wp], host + (size_t)r * t.cols + (size_t)ch * t.chunk_w,
             sizeof(float) * t.chunk_w);
}
void unpack(const TensorInfo& t, const std::vector<float>& dev, float* host, float scale) {
  for (int r = 0; r < t.rows; ++r)
    for (int ch = 0; ch < t.chunks; ++ch)
      for (int j = 0; j < t.chunk_w; ++j)
        host[(size_t)r * t.cols + (size_t)ch * t.chunk_w + j] = dev[(size_t)r * t.ld + (size_t)ch * t.chunk_wp + j] * scale;
}

}  // namespace smx

// ---- developer knobs (smx_internal.h: tuning) -----------------------------------------------------------------------------
namespace smx {
static std::mutex g_tuning_mu;
static std::map<std::string, double>& tuning_map() {
  static std::map<std::string, double> mp;
  static bool parsed = false;
  if (!parsed) {   // SMX_TUNING="name=value,name=value" (a bare name means 1)
    parsed = true;
    if (const char* e = getenv("SMX_TUNING")) {
      std::string str(e);
      size_t i = 0;
      while (i < str.size()) {
        size_t j = str.find(',', i);
        if (j == std::string::npos) j = str.size();
        const std::string item = str.substr(i, j - i);
        const size_t eq = item.find('=');
        if (!item.empty()) mp[item.substr(0, eq)] = eq == std::string::npos ? 1.0 : atof(item.c_str() + eq + 1);
        i = j + 1;
      }
    }
  }
  return mp;
}
// moves on whenever a knob is set or cleared: anything cached under the knobs in force (the scoring head's W images: ADVICE r05) is keyed by it
std::atomic<unsigned long long> g_tuning_epoch{1};
unsigned long long tuning_epoch() { return g_tuning_epoch.load(); }
double tuning(const char* name, double dflt) {
  std::lock_guard<std::mutex> lk(g_tuning_mu);
  auto& mp = tuning_map();
  auto it = mp.find(name);
  return it == mp.end() ? dflt : it->second;
}
}  // namespace smx

namespace smx {

// the buffers with one row per row of a pass (what alloc_rows owns)
static std::vector<void**> row_buffers(smx_model* m) {
  std::vector<void**> v;
  auto add = [&](auto*& p) { v.push_back(reinterpret_cast<void**>(&p)); };
  for (auto* mlp : {&m->enc, &m->encl, &m->dec})
    for (auto& L : *mlp) { add(L.xhat); add(L.out_buf); add(L.dpre); add(L.inv_std); add(L.noise); }
  add(m->bigk_part); add(m->slab); add(m->latbuf); add(m->dlat); add(m->z); add(m->noise_eps); add(m->sig); add(m->eps); add(m->kl);
  add(m->P); add(m->dP); add(m->llk_part); add(m->llk_y); add(m->llk_o); add(m->rows2[0]); add(m->rows2[1]);
  add(m->resp); add(m->dklz); add(m->tril_part); add(m->zmean); add(m->zpick); add(m->ltril);
  add(m->raw); add(m->draw); add(m->rho); add(m->latlbuf); add(m->dlatl); add(m->lsmp); add(m->lsig); add(m->leps); add(m->kl_l); add(m->dl);
  for (int j = 0; j < SMX_MAX_LABELS; ++j) { add(m->laby_raw[j]); add(m->laby_draw[j]); }
  if (m->x_csr) add(m->xbatch);
  return v;
}

// allocates every row buffer for R rows into the (null) pointers of row_buffers.  Knob alloc_rows_fail = n (test hook): the n-th
// allocation reports SMX_ERR_NOMEM, as a hipMalloc beyond the device's memory would
static int alloc_rows_into(smx_model* m, size_t R) {
  const smx_config* cfg = &m->cfg;
  const size_t B = R;
  const int fail_at = (int)tuning("alloc_rows_fail", 0.0);
  int n_alloc = 0;
  auto dm = [&](auto** p, size_t n) -> int {
    if (fail_at > 0 && ++n_alloc >= fail_at) { set_error("hipMalloc failed: out of memory (knob alloc_rows_fail)"); return SMX_ERR_NOMEM; }
    return dmalloc(p, n);
  };
  int rc = SMX_OK;
  if (m->x_csr && (rc = dm(&m->xbatch, B * m->Gp))) return rc;
  m->max_feat_p = m->Dp;
  auto alloc_mlp = [&](std::vector<MlpLayer>& mlp) {
    for (auto& L : mlp) {
      if (L.out_p > m->max_feat_p) m->max_feat_p = L.out_p;
      if ((rc = dm(&L.xhat, B * L.out_p))) return rc;
      if ((rc = dm(&L.out_buf, B * L.out_p))) return rc;
      if ((rc = dm(&L.dpre, B * L.out_p))) return rc;
      if ((rc = dm(&L.inv_std, (size_t)L.out_p))) return rc;
      if ((rc = dm(&L.noise, B * L.out_p))) return rc;
    }
    return (int)SMX_OK;
  };
  if ((rc = alloc_mlp(m->enc)) || (rc = alloc_mlp(m->encl)) || (rc = alloc_mlp(m->dec))) return rc;
  for (auto& L : m->disc) if (L.out_p > m->max_feat_p) m->max_feat_p = L.out_p;
  const size_t lat_ld = (size_t)m->lat_planes * (size_t)m->Dp;
  const size_t ldp = (size_t)m->k * m->Gp;
  // wide panels: scratch for the per-slice slabs of the products that contract over the gene axis (smx_bigk.hip)
  if (m->Gp >= std::min(4096, head_fused_min_genes())) {
    if ((rc = dm(&m->bigk_part, (size_t)SMX_BIGK_MAX_SLICES * B * m->max_feat_p))) return rc;
    if (!m->hf_tab) {   // (not a row buffer: allocated once, at model creation)
      float* tab = nullptr;
      if ((rc = dmalloc(&tab, (size_t)SMX_HEAD_FUSED_TAB_BYTES / 4))) return rc;
      m->hf_tab = tab;
      if ((rc = head_fused_prepare())) return rc;
    }
  }
  if ((rc = dm(&m->slab, (size_t)(64 * 3 + SMX_MAX_LABELS + 1) * B * m->max_feat_p)) || (rc = dm(&m->latbuf, B * lat_ld)) || (rc = dm(&m->dlat, B * lat_ld)) ||
      (rc = dm(&m->z, B * m->Dp)) || (rc = dm(&m->noise_eps, B * m->Dp)) || (rc = dm(&m->sig, B * m->Dp)) || (rc = dm(&m->eps, B * m->Dp)) ||
      (rc = dm(&m->kl, B)) || (rc = dm(&m->P, B * ldp)) || (rc = dm(&m->dP, B * ldp)) ||
      (rc = dm(&m->llk_part, B * (size_t)std::max(std::max(loss_chunks_max(m->Gp), head_loss_chunks(m->Gp)), 256))) || (rc = dm(&m->llk_y, B)) || (rc = dm(&m->llk_o, B)) ||
      (rc = dm(&m->rows2[0], B)) || (rc = dm(&m->rows2[1], B)))
    return rc;
  if (m->scale && ((rc = dm(&m->resp, B * 32)) || (rc = dm(&m->dklz, B * m->Dp)))) return rc;
  if (m->scale_tril && (rc = dm(&m->tril_part, (size_t)cfg->n_components * ((B + 7) / 8) * m->D * (m->D + 2)))) return rc;
  if (m->mixpost && ((rc = dm(&m->resp, B * 32)) || (rc = dm(&m->zmean, B * m->Dp)) || (rc = dm(&m->zpick, B)))) return rc;
  if (m->latent_tril && (rc = dm(&m->ltril, B * (size_t)m->D * m->D))) return rc;
  if (m->scvi) {
    if ((rc = dm(&m->raw, B * ldp)) || (rc = dm(&m->draw, B * ldp)) || (rc = dm(&m->rho, B * m->Gp)) ||
        (rc = dm(&m->latlbuf, B * 32)) || (rc = dm(&m->dlatl, B * 32)) || (rc = dm(&m->lsmp, B)) ||
        (rc = dm(&m->lsig, B)) || (rc = dm(&m->leps, B)) || (rc = dm(&m->kl_l, B)) || (rc = dm(&m->dl, B)))
      return rc;
  }
  for (int j = 0; j < m->n_heads; ++j) {
    const size_t ld = m->tensors[m->t_labW[j]].ld;
    if ((rc = dm(&m->laby_raw[j], B * ld)) || (rc = dm(&m->laby_draw[j], B * ld))) return rc;
  }
  return SMX_OK;
}

// smx_set_optimizer's hyper-parameters with the defaults filled in (Adam's from `adam_hp`: the config's beta_1, beta_2, epsilon), checked
int opt_resolve(int rule, const float* hp, int n_hp, const float* adam_hp, float out[4]) {
  static const float defaults[5][4] = {{0.9f, 0.999f, 1e-7f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.9f, 0.f, 1e-7f, 0.f}, {0.1f, 1e-7f, 0.f, 0.f},
                                       {0.9f, 0.999f, 1e-7f, 0.f}};
  static const int counts[5] = {3, 2, 3, 2, 3};
  SMX_REQUIRE(rule >= 0 && rule <= 4, "smx_set_optimizer: unknown rule (SMX_OPT_ADAM, SGD, RMSPROP, ADAGRAD, ADAMAX)");
  SMX_REQUIRE(n_hp >= 0 && n_hp <= counts[rule] && (n_hp == 0 || hp), "smx_set_optimizer: too many hyper-parameters for the rule");
  for (int i = 0; i < 4; ++i) out[i] = i < n_hp ? hp[i] : (rule == 0 && i < 3 ? adam_hp[i] : defaults[rule][i]);
  for (int i = 0; i < counts[rule]; ++i) SMX_REQUIRE(std::isfinite(out[i]), "smx_set_optimizer: a hyper-parameter is not finite");
  switch (rule) {
    // epsilon a NORMAL float32 (>= 2^-126): a tensor's padding has g = m = v = 0, and at epsilon 0 every rule with a quotient makes
    // -(lr 0) * (1 / (sqrt(0) + 0)) = 0 * inf = NaN of it -- padding the products read as operands and smx_model.h requires to be zero
    // (DESIGN.md 4w).  A denormal epsilon does the same: its reciprocal is beyond float32, and v_rcp_f32 reads a denormal operand as 0.
    // Adagrad's accumulator starts at its initial value in the logical elements only, so its padding needs this whatever that value is.
    case 0: case 4: SMX_REQUIRE(out[0] >= 0.f && out[0] < 1.f && out[1] >= 0.f && out[1] < 1.f && out[2] >= FLT_MIN, "smx_set_optimizer: beta_1, beta_2 in [0, 1), epsilon a normal float32 (>= 2^-126)"); break;
    case 1: SMX_REQUIRE(out[0] >= 0.f && (out[1] == 0.f || out[1] == 1.f), "smx_set_optimizer: sgd momentum >= 0, nesterov 0 or 1"); break;
    case 2: SMX_REQUIRE(out[0] >= 0.f && out[0] <= 1.f && out[1] >= 0.f && out[2] >= FLT_MIN, "smx_set_optimizer: rmsprop rho in [0, 1], momentum >= 0, epsilon a normal float32 (>= 2^-126)"); break;
    case 3: SMX_REQUIRE(out[0] >= 0.f && out[1] >= FLT_MIN, "smx_set_optimizer: adagrad initial_accumulator_value >= 0, epsilon a normal float32 (>= 2^-126)"); break;
  }
  return SMX_OK;
}
void opt_scalars(int rule, const float hp[4], AdamArgs& a) {
  a.momentum = 0.f;
  switch (rule) {
    case 1: a.momentum = hp[0]; a.form = hp[0] == 0.f ? OPT_SGD : (hp[1] != 0.f ? OPT_SGD_NESTEROV : OPT_SGD_MOM); break;
    case 2: a.b1 = hp[0]; a.momentum = hp[1]; a.eps = hp[2]; a.form = hp[1] == 0.f ? OPT_RMSPROP : OPT_RMSPROP_MOM; break;
    case 3: a.eps = hp[1]; a.form = OPT_ADAGRAD; break;
    case 4: a.b1 = hp[0]; a.b2 = hp[1]; a.eps = hp[2]; a.form = OPT_ADAMAX; break;
    default: a.b1 = hp[0]; a.b2 = hp[1]; a.eps = hp[2]; a.form = OPT_ADAM; break;
  }
}

// Every buffer with one row per row of a pass, for R rows: at model creation R = max_batch; smx_set_train_draws regrows them to
// draws x max_batch (the stacked rows of a multi-draw step).  All or nothing: the new set is allocated beside the old one, which is
// freed only when every allocation succeeded; on failure the model keeps its previous buffers and Rmax.  The caller has synchronised
// and sets the routing capacities (set_row_caps).
int alloc_rows(smx_model* m, size_t R) {
  const std::vector<void**> bufs = row_buffers(m);
  std::vector<void*> old(bufs.size());
  for (size_t i = 0; i < bufs.size(); ++i) { old[i] = *bufs[i]; *bufs[i] = nullptr; }
  const int rc = alloc_rows_into(m, R);
  for (size_t i = 0; i < bufs.size(); ++i) {
    void* drop = rc == SMX_OK ? old[i] : *bufs[i];
    if (rc != SMX_OK) *bufs[i] = old[i];
    if (drop) hipFree(drop);
  }
  if (rc != SMX_OK) return rc;
  m->Rmax = (int)R;
  if (m->x_csr) m->X = m->xbatch;   // (the sparse store: m->X aliases its expansion tile)
  return SMX_OK;
}

// The capacities the routing predicates of smx_forward.hip and smx_backward.hip read (slab / bigk scratch, the tril prior's partials), for `rows` rows of a
// pass -- max_batch at one draw, draws x max_batch otherwise -- not the allocation's: an engine grown for several draws and set back to
// one routes exactly as a fresh engine.  rows <= Rmax.
void set_row_caps(smx_model* m, size_t rows) {
  m->slab_cap = (size_t)(64 * 3 + SMX_MAX_LABELS + 1) * rows * m->max_feat_p;
  m->bigk_floats = m->bigk_part ? (size_t)SMX_BIGK_MAX_SLICES * rows * m->max_feat_p : 0;
  m->tril_part_floats = m->scale_tril ? (size_t)m->cfg.n_components * ((rows + 7) / 8) * m->D * (m->D + 2) : 0;
}

}  // namespace smx

extern "C" {

const char* smx_last_error(void) { return last_error_cstr(); }
int smx_abi_version(void) { return SMX_ABI_VERSION; }

// Host-side helper (no device work): the visit order of one epoch under a streaming shuffle buffer, the sequential part
// of sisua_amd/data.py::epoch_order (tf.data's .shuffle(buffer) semantics, _single_cell_base.py:597-600).  picks[t] are
// the caller's random integers (NumPy RandomState stream: the order is defined there); 2.3 ms per 3381-cell epoch in
// Python -- as long as the device needs for the epoch itself -- against ~10 us here.
int smx_shuffle_order(int32_t n_obs, int32_t buffer, const int64_t* picks, int32_t* out) {
  SMX_REQUIRE(n_obs >= 0 && buffer > 0 && (n_obs == 0 || (picks && out)), "bad arguments");
  std::vector<int32_t> buf((size_t)std::min(buffer, n_obs));
  for (size_t i = 0; i < buf.size(); ++i) buf[i] = (int32_t)i;
  int32_t nxt = (int32_t)buf.size();
  size_t len = buf.size();
  for (int32_t t = 0; t < n_obs; ++t) {
    SMX_REQUIRE(picks[t] >= 0 && len > 0, "negative pick");
    const size_t k = (size_t)(picks[t] % (int64_t)len);
    out[t] = buf[k];
    if (nxt < n_obs) buf[k] = nxt++;
    else { buf[k] = buf[len - 1]; --len; }
  }
  return SMX_OK;
}

int smx_set_tuning(const char* name, double value) {
  SMX_REQUIRE(name && *name, "null name");
  std::lock_guard<std::mutex> lk(smx::g_tuning_mu);
  smx::tuning_map()[name] = value;
  ++smx::g_tuning_epoch;
  return SMX_OK;
}
int smx_clear_tuning(const char* name) {
  std::lock_guard<std::mutex> lk(smx::g_tuning_mu);
  if (name && *name) smx::tuning_map().erase(name); else smx::tuning_map().clear();
  ++smx::g_tuning_epoch;
  return SMX_OK;
}

int smx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int smx_init(int device) {
  int n = smx_device_count();
  if (device < 0 || device >= n) {
    set_error("smx_init: no such HIP device (" + std::to_string(device) + " of " + std::to_string(n) + ")");
    return SMX_ERR_INVALID;
  }
  SMX_HIP(hipSetDevice(device));
  return SMX_OK;
}

int smx_synchronize(void) {
  SMX_HIP(hipDeviceSynchronize());
  return SMX_OK;
}

int smx_model_create(const smx_config* cfg, smx_model** out) {
  SMX_REQUIRE(cfg && out, "null argument");
  SMX_REQUIRE(cfg->abi_version == SMX_ABI_VERSION, "smx_config.abi_version mismatch");
  SMX_REQUIRE(cfg->n_genes > 0 && cfg->latent_dim > 0 && cfg->max_batch > 0, "n_genes, latent_dim, max_batch must be > 0");
  SMX_REQUIRE(cfg->n_enc >= 1 && cfg->n_enc <= SMX_MAX_LAYERS && cfg->n_dec >= 1 && cfg->n_dec <= SMX_MAX_LAYERS,
              "encoder/decoder need 1..8 layers");
  SMX_REQUIRE(cfg->model >= SMX_MODEL_VAE && cfg->model <= SMX_MODEL_SCALE_POST, "unknown model kind");
  if (cfg->model == SMX_MODEL_FVAE) {
    SMX_REQUIRE(cfg->disc_layers >= 1 && cfg->disc_layers <= SMX_MAX_LAYERS && cfg->disc_units >= 1, "fvae: discriminator needs 1..8 hidden layers");
    SMX_REQUIRE(cfg->disc_leak >= 0.f && cfg->disc_leak < 1.f, "fvae: leaky-ReLU slope in [0, 1)");
  }
  if (cfg->model == SMX_MODEL_SCALE || cfg->model == SMX_MODEL_SCALE_TRIL) SMX_REQUIRE(cfg->n_components >= 2 && cfg->n_components <= 32, "scale: 2..32 mixture components");
  if (cfg->model == SMX_MODEL_SCALE_TRIL) SMX_REQUIRE(cfg->latent_dim <= 32, "scale with full-covariance components: at most 32 latent dimensions");
  if (cfg->model == SMX_MODEL_SCALE_POST) SMX_REQUIRE(cfg->n_components >= 2 && cfg->n_components <= 8 && cfg->n_components <= cfg->latent_dim && cfg->latent_dim <= 64, "scale with a mixture-density posterior: 2 .. min(latent_dim, 8) components, at most 64 latent dimensions");
  SMX_REQUIRE(cfg->likelihood >= SMX_LLK_NB && cfg->likelihood <= SMX_LLK_NORMAL, "unknown likelihood");
  SMX_REQUIRE(cfg->n_labels >= 0 && cfg->n_labels <= SMX_MAX_LABELS, "too many label heads");
  // (SCALE with label heads = SCALAR, sisua/models/scale.py:52-59: the mixture prior of SCALE under SISUA's semi-supervised heads)
  int n_observed = 0;
  for (int j = 0; j < cfg->n_labels; ++j) {
    if (cfg->label_observed[j]) { SMX_REQUIRE(j == n_observed, "observed output heads come before the label heads"); ++n_observed; }
  }
  // (outputs[1:], tests/test_singlecell_models.py:129-141 / scvi.py:168-169: observed heads on any model's decoder output -- FactorVAE
  // (fvae.py:9-18 passes `outputs` through unchanged) and the mixture-density posterior included since round 5)
  if (cfg->model == SMX_MODEL_FVAE) {   // SemiFVAE's label variables (behind the observed outputs) are classified by the discriminator: no heads
    SMX_REQUIRE(cfg->n_labels - n_observed <= SMX_DISC_MAX_GROUPS, "fvae: at most 8 label variables");
    int classes = 0;
    for (int j = n_observed; j < cfg->n_labels; ++j) {
      SMX_REQUIRE(cfg->label_llk[j] == SMX_LABEL_ONEHOT && cfg->label_dim[j] >= 2, "fvae: label variables are one-hot with at least 2 classes");
      classes += cfg->label_dim[j];
    }
    SMX_REQUIRE(classes <= 32, "fvae: the label variables have at most 32 classes in all (the discriminator's logit layer)");
  }
  if (cfg->latent_tril) {
    SMX_REQUIRE(cfg->model == SMX_MODEL_VAE || cfg->model == SMX_MODEL_SISUA || cfg->model == SMX_MODEL_SCVI,
                "latent_tril: the full-covariance posterior is built for VAE, SISUA / MISA and SCVI");
    SMX_REQUIRE(cfg->latent_dim >= 1 && cfg->latent_dim <= 32, "latent_tril: 1 <= latent_dim <= 32");
  }
  if (cfg->model == SMX_MODEL_SCALE_POST) SMX_REQUIRE(cfg->n_labels == n_observed, "scale with a mixture-density posterior: no label heads (observed outputs only)");
  SMX_REQUIRE(cfg->model == SMX_MODEL_SISUA || cfg->model == SMX_MODEL_FVAE || cfg->model == SMX_MODEL_SCALE || cfg->model == SMX_MODEL_SCALE_TRIL || cfg->n_labels == n_observed,
              "label heads need model = SISUA, SCALE (SCALAR) or FVAE (SemiFVAE)");
  SMX_REQUIRE(cfg->scvi_dispersion >= 0 && cfg->scvi_dispersion <= 2 && cfg->scvi_inflation >= 0 && cfg->scvi_inflation <= 2, "scvi_dispersion / scvi_inflation: 0 ('full'), 1 ('share') or 2 ('single')");
  SMX_REQUIRE(cfg->model == SMX_MODEL_SCVI || (cfg->scvi_dispersion == 0 && cfg->scvi_inflation == 0), "dispersion / inflation are options of scvi");
  if (cfg->model == SMX_MODEL_SCVI) {
    SMX_REQUIRE(cfg->likelihood == SMX_LLK_NBD || cfg->likelihood == SMX_LLK_ZINBD, "scvi supports nbd / zinbd only");
    SMX_REQUIRE(cfg->n_encl >= 1 && cfg->n_encl <= SMX_MAX_LAYERS, "scvi needs a library encoder");
  }
  SMX_REQUIRE(cfg->dropout_enc >= 0 && cfg->dropout_enc < 1 && cfg->dropout_dec >= 0 && cfg->dropout_dec < 1 &&
                  cfg->input_dropout >= 0 && cfg->input_dropout < 1, "dropout rates must be in [0,1)");
  SMX_REQUIRE(cfg->adam_eps >= FLT_MIN, "adam_eps must be a normal float32 (>= 2^-126; below, the update turns every tensor's zero padding into NaN: opt_resolve)");
  int dev = 0;
  SMX_HIP(hipGetDevice(&dev));
  smx_model* m = new smx_model();
  m->cfg = *cfg; m->device = dev;
  m->opt_hp[0] = cfg->adam_beta1; m->opt_hp[1] = cfg->adam_beta2; m->opt_hp[2] = cfg->adam_eps;   // (SMX_OPT_ADAM, t0 = 0)
  m->G = cfg->n_genes; m->Gp = round_up(m->G, 32); m->D = cfg->latent_dim; m->Dp = round_up(m->D, 32);
  m->k = llk_planes(cfg->likelihood);
  m->stochastic = cfg->model != SMX_MODEL_DCA; m->scvi = cfg->model == SMX_MODEL_SCVI; m->scale = cfg->model == SMX_MODEL_SCALE || cfg->model == SMX_MODEL_SCALE_TRIL; m->scale_tril = cfg->model == SMX_MODEL_SCALE_TRIL;
  m->mixpost = cfg->model == SMX_MODEL_SCALE_POST;
  m->latent_tril = cfg->latent_tril != 0;
  m->lat_planes = m->mixpost ? 1 + 2 * cfg->n_components : m->latent_tril ? 1 + cfg->latent_dim : (m->stochastic ? 2 : 1);
  m->fvae = cfg->model == SMX_MODEL_FVAE; m->n_heads = m->fvae ? n_observed : cfg->n_labels; m->n_observed = n_observed;
  m->out_has_W[1] = cfg->scvi_dispersion == 0; m->out_has_W[2] = cfg->scvi_inflation == 0;
  m->out_single[1] = cfg->scvi_dispersion == 2; m->out_single[2] = cfg->scvi_inflation == 2;
  m->Bmax = cfg->max_batch;
  int rc = SMX_OK;
  auto fail = [&](int code) { smx_model_destroy(m); return code; };
  if (hipStreamCreate(&m->st) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(SMX_ERR_HIP); }
  // ---- manifest (same order as oracle/sisua_oracle.py:manifest) ----
  const bool bnorm = cfg->batchnorm != 0;
  int h = build_mlp(m, m->enc, "enc", m->G, cfg->n_enc, cfg->enc_units, ST_ENC_DROPOUT, cfg->dropout_enc, bnorm);
  m->t_latW = add_tensor(m, "lat/W", h, m->lat_planes * m->D, m->lat_planes, false);
  m->t_latb = add_tensor(m, "lat/b", 1, m->lat_planes * m->D, m->lat_planes, true);
  if (m->scale) {   // trainable mixture prior: logits [C], means and raw scales [C][D]
    m->t_prLogits = add_tensor(m, "prior/logits", 1, cfg->n_components, 1, true);
    m->t_prLoc = add_tensor(m, "prior/loc", cfg->n_components, m->D, 1, false);
    m->t_prScale = add_tensor(m, "prior/scale", m->scale_tril ? cfg->n_components * m->D : cfg->n_components, m->D, 1, false);   // (tril: row c D + p = row p of L_c)
  }
  if (m->scvi) {
    int hl = build_mlp(m, m->encl, "encl", m->G, cfg->n_encl, cfg->encl_units, ST_ENCL_DROPOUT, cfg->dropout_enc, bnorm);
    m->t_latlW = add_tensor(m, "latl/W", hl, 2, 1, false);
    m->t_latlb = add_tensor(m, "latl/b", 1, 2, 1, true);
  }
  int hd = build_mlp(m, m->dec, "dec", m->D, cfg->n_dec, cfg->dec_units, ST_DEC_DROPOUT, cfg->dropout_dec, bnorm);
  if (m->fvae) {   // discriminator: Dense + bias + leaky ReLU, never BatchNorm / dropout; then the logit layer
    int32_t du[SMX_MAX_LAYERS];
    for (int i = 0; i < cfg->disc_layers; ++i) du[i] = cfg->disc_units;
    const int hu = build_mlp(m, m->disc, "disc", m->D, cfg->disc_layers, du, 0, 0.f, false, cfg->disc_leak);
    int n_out = cfg->n_labels > n_observed ? 0 : 1;   // (the label variables sit behind the observed outputs in the target order)
    for (int j = n_observed; j < cfg->n_labels; ++j) { n_out += cfg->label_dim[j]; m->lab_Pp[j] = round_up(cfg->label_dim[j], 32); }
    m->t_discoutW = add_tensor(m, "discout/W", hu, n_out, 1, false);
    m->t_discoutb = add_tensor(m, "discout/b", 1, n_out, 1, true);
  }
  if (m->scvi) {
    for (int ch = 0; ch < m->k; ++ch) {   // (scvi.py:66-86: no Dense head for a 'share'd plane -- its per-gene vector is out{ch}/b alone)
      if (m->out_has_W[ch]) m->t_outW[ch] = add_tensor(m, "out" + std::to_string(ch) + "/W", hd, m->G, 1, false);
      m->t_outb[ch] = add_tensor(m, "out" + std::to_string(ch) + "/b", 1, m->out_single[ch] ? 1 : m->G, 1, true);   // ('single': one scalar)
    }
  } else {
    m->t_outW[0] = add_tensor(m, "out/W", hd, m->k * m->G, m->k, false);
    m->t_outb[0] = add_tensor(m, "out/b", 1, m->k * m->G, m->k, true);
  }
  for (int j = 0; j < m->n_heads; ++j) {
    SMX_REQUIRE(cfg->label_dim[j] > 0, "label_dim must be > 0");
    SMX_REQUIRE(cfg->label_llk[j] >= SMX_LABEL_NB && cfg->label_llk[j] <= SMX_LABEL_NORMAL, "unknown label likelihood");
    if (cfg->label_llk[j] >= SMX_LABEL_MIXNB && cfg->label_llk[j] <= SMX_LABEL_MIXZINB) SMX_REQUIRE(cfg->label_components[j] >= 2 && cfg->label_components[j] <= 4, "mixture label heads have 2..4 components");
    if (cfg->label_llk[j] == SMX_LABEL_MIXTRIL) SMX_REQUIRE(cfg->label_dim[j] <= 64, "'mixtril' label heads take at most 64 label dimensions");
    // planes of the head: (log total_count, logits) | logits | C x (mixture logit, two component parameters) | 'mixtril': C mixture-logit
    // planes, C location planes, C x P planes = the columns of the components' scale factors (label_tril_kernel) | 'bernoulli': logits |
    // 'normal': (loc, raw scale)
    m->lab_ky[j] = (cfg->label_llk[j] == SMX_LABEL_NB || cfg->label_llk[j] == SMX_LABEL_NBD || cfg->label_llk[j] == SMX_LABEL_NORMAL) ? 2 :
                   (cfg->label_llk[j] == SMX_LABEL_ZINB || cfg->label_llk[j] == SMX_LABEL_ZINBD) ? 3 :
                   (cfg->label_llk[j] == SMX_LABEL_ONEHOT || cfg->label_llk[j] == SMX_LABEL_BERNOULLI) ? 1 :
                   cfg->label_llk[j] == SMX_LABEL_MIXTRIL ? cfg->label_components[j] * (2 + cfg->label_dim[j]) :
                   cfg->label_llk[j] == SMX_LABEL_MIXZINB ? 4 * cfg->label_components[j] : 3 * cfg->label_components[j];
    m->lab_Pp[j] = round_up(cfg->label_dim[j], 32);
    m->t_labW[j] = add_tensor(m, "lab" + std::to_string(j) + "/W", hd, m->lab_ky[j] * cfg->label_dim[j], m->lab_ky[j], false);
    m->t_labb[j] = add_tensor(m, "lab" + std::to_string(j) + "/b", 1, m->lab_ky[j] * cfg->label_dim[j], m->lab_ky[j], true);
  }
  // ---- flat buffers ----
  // layout: [encoder / latent / decoder tensors | tail: BN batch stats, metrics | output + label heads].
  // The head gradients (3/4 of the bytes) are produced by the FIRST backward launch, so under data
  // parallelism that contiguous bucket is all-reduced on a communication stream while the rest of
  // the backward pass runs; the front bucket (with the tail) follows when backward is done.
  size_t off = 0;
  for (size_t i = 0; i < m->bn_w.size(); ++i) { m->bn_off.push_back(off); off += 2 * (size_t)m->bn_wp[i]; }
  m->bn_total = off;
  {
    auto is_head = [](const std::string& n) { return n.compare(0, 3, "out") == 0 || n.compare(0, 3, "lab") == 0; };
    size_t cur = 0;
    for (auto& t : m->tensors) if (!is_head(t.name)) { t.offset = cur; cur += (t.count + 63) / 64 * 64; }
    m->tail_off_bn = cur;
    m->tail_off_metrics = m->tail_off_bn + (m->bn_total + 63) / 64 * 64;
    cur = m->tail_off_metrics + 64;
    m->bucket1_off = cur;
    for (auto& t : m->tensors) if (is_head(t.name)) { t.offset = cur; cur += (t.count + 63) / 64 * 64; }
    m->bucket1_count = cur - m->bucket1_off;
    m->flat_count = cur;
    m->grads_count = cur;
  }
  // (SMX_SHARD_SLACK floats behind the head bucket: flag opt_shard cuts the bucket into world slices of equal, 64-float-aligned length)
  if ((rc = dmalloc(&m->params, m->flat_count + SMX_SHARD_SLACK))) return fail(rc);
  if ((rc = dmalloc(&m->grads, m->grads_count + SMX_SHARD_SLACK))) return fail(rc);
  if ((rc = dmalloc(&m->adam_m, m->flat_count + SMX_SHARD_SLACK))) return fail(rc);
  if ((rc = dmalloc(&m->adam_v, m->flat_count + SMX_SHARD_SLACK))) return fail(rc);
  if ((rc = dmalloc(&m->bn_moving, m->bn_total))) return fail(rc);
  {  // moving variance starts at 1 (Keras)
    std::vector<float> init(m->bn_total, 0.f);
    for (size_t i = 0; i < m->bn_w.size(); ++i)
      for (int j = 0; j < m->bn_wp[i]; ++j) init[m->bn_off[i] + m->bn_wp[i] + j] = 1.f;
    if (m->bn_total && hipMemcpy(m->bn_moving, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("bn init copy failed"); return fail(SMX_ERR_HIP);
    }
  }
  // ---- activations ----
  const size_t B = m->Bmax;
  if (m->fvae) {   // the discriminator sees the stacked batch [z ; z_perm]: 2 B rows
    int up = 32;
    for (auto& L : m->disc) {
      up = std::max(up, L.out_p);
      if ((rc = dmalloc(&L.xhat, 2 * B * L.out_p)) || (rc = dmalloc(&L.out_buf, 2 * B * L.out_p)) || (rc = dmalloc(&L.dpre, 3 * B * L.out_p)))   // (d pre: both backward sweeps as rows of one buffer)
        return fail(rc);
    }
    // the two upstream gradients on the logits in ONE buffer: rows [0, 2B) the discriminator's objective, rows [2B, 3B) the TC term
    if ((rc = dmalloc(&m->zz, 2 * B * m->Dp)) || (rc = dmalloc(&m->u_d, 3 * B * 32)) ||
        (rc = dmalloc(&m->tc_cell, B)) || (rc = dmalloc(&m->dl_cell, 2 * B)) || (rc = dmalloc(&m->dz_tc, B * m->Dp)) ||
        (rc = dmalloc(&m->disc_dpre, B * up)) || (rc = dmalloc(&m->disc_db, (size_t)up)))
      return fail(rc);
  }
  if ((rc = dmalloc(&m->state3, (size_t)3)) || (rc = dmalloc(&m->hostX, B * m->Gp)) || (rc = dmalloc(&m->hostLib, B * 2)) ||
      (rc = dmalloc(&m->hostLgx1, B)) || (rc = alloc_rows(m, B)))
    return fail(rc);
  if (!llk_has_count_const(cfg->likelihood)) {
    if ((rc = dmalloc(&m->zero_rows, B))) return fail(rc);
    if (hipMemset(m->zero_rows, 0, B * sizeof(float)) != hipSuccess) { set_error("zero_rows: hipMemset failed"); return fail(SMX_ERR_HIP); }
  }
  set_row_caps(m, B);
  // ---- optimiser chunk table ----
  std::vector<OptChunk> chunks;
  // floats per optimiser workgroup
  const int CH = 4096;
  for (size_t t = 0; t < m->tensors.size(); ++t) {
    const TensorInfo& ti = m->tensors[t];
    const int first = (int)chunks.size();
    const int n = (int)((ti.count + CH - 1) / CH);
    for (int i = 0; i < n; ++i) {
      OptChunk c;
      memset(&c, 0, sizeof(c));
      c.tensor = (int)t; c.offset = (int)(ti.offset + (size_t)i * CH);
      c.count = (int)((size_t)(i + 1) * CH <= ti.count ? CH : ti.count - (size_t)i * CH);
      c.first_chunk = first; c.n_chunks = n; c.tensor_count = (int32_t)ti.count;
      chunks.push_back(c);
    }
  }
  m->n_chunks = (int)chunks.size();
  m->chunks_floats = CH;
  m->chunk_first_head = m->n_chunks;
  for (size_t i = 0; i < chunks.size(); ++i)
    if (chunks[i].tensor == m->t_outW[0]) { m->chunk_first_head = (int)i; break; }
  m->chunk_first_label = m->n_chunks;
  if (m->n_heads > 0)
    for (size_t i = 0; i < chunks.size(); ++i)
      if (chunks[i].tensor == m->t_labW[0]) { m->chunk_first_label = (int)i; break; }
  if (m->tensors.size() <= SMX_MAX_TENSORS) {   // slots for the products' sum-of-squares partials (32 x 32 tiles at most)
    size_t total = 0;
    m->sq_first.assign(m->tensors.size(), 0);
    m->sq_count.assign(m->tensors.size(), 0);
    for (size_t t = 0; t < m->tensors.size(); ++t) {
      const TensorInfo& ti = m->tensors[t];
      m->sq_first[t] = (int)total;
      total += (size_t)((ti.rows_p + 31) / 32) * (size_t)((ti.ld + 31) / 32) * 8;   // (the wide head-backward kernel leaves 8 per tile when the planes are separate tensors)
    }
    m->sq_total_first = (int)total;   // SMX_SQR_PER_TENSOR more slots per tensor: the sums the reduce riders leave (attach_early_adam)
    m->sq_reduced.assign(m->tensors.size(), 0);
    if ((rc = dmalloc(&m->sq_slots, total + m->tensors.size() * SMX_SQR_PER_TENSOR))) return fail(rc);
  }
  if ((rc = dmalloc(&m->chunks, chunks.size())) || (rc = dmalloc(&m->partial, chunks.size())) || (rc = dmalloc(&m->shard_partial, chunks.size())) ||
      (rc = dmalloc(&m->tensor_norm, m->tensors.size())))
    return fail(rc);
  if (hipMemcpy(m->chunks, chunks.data(), chunks.size() * sizeof(OptChunk), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("chunk table copy failed"); return fail(SMX_ERR_HIP);
  }
  *out = m;
  return SMX_OK;
}

int smx_model_destroy(smx_model* m) {
  if (!m) return SMX_OK;
  if (m->st) hipStreamSynchronize(m->st);
  for (auto& kv : m->graphs) hipGraphExecDestroy(kv.second);
  for (auto& ev : m->timing_events) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
  if (m->bigk_part) hipFree(m->bigk_part);
  if (m->hf_tab) hipFree(m->hf_tab);
  p2p_release(m);
  if (m->comm2 && g_rccl.CommDestroy) g_rccl.CommDestroy(m->comm2);   // (the heads' bucket's communicator: a split of `comm`, destroyed first)
  m->comm2 = nullptr;
  if (m->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(m->comm);
  m->comm = nullptr;
  m->local.reset();
  auto fr = [](void* p) { if (p) hipFree(p); };
  fr(m->local_scratch); fr(m->sync_buf);
  fr(m->params); fr(m->grads); fr(m->adam_m); fr(m->adam_v); fr(m->bn_moving);
  for (auto* mlp : {&m->enc, &m->encl, &m->dec})
    for (auto& L : *mlp) { fr(L.xhat); fr(L.out_buf); fr(L.dpre); fr(L.inv_std); fr(L.noise); }
  release_dataset(m);
  fr(m->hostX); fr(m->hostLib); fr(m->hostLgx1); fr(m->zero_rows);
  for (int j = 0; j < SMX_MAX_LABELS; ++j) { fr(m->laby_raw[j]); fr(m->laby_draw[j]); }
  fr(m->rows2[0]); fr(m->rows2[1]); fr(m->order); fr(m->sched_tab); fr(m->state3); fr(m->mhist);
  fr(m->resp); fr(m->dklz); fr(m->zmean); fr(m->zpick); fr(m->tril_part); fr(m->ltril);
  for (auto& L : m->disc) { fr(L.xhat); fr(L.out_buf); fr(L.dpre); }
  fr(m->zz); fr(m->u_d); fr(m->tc_cell); fr(m->dl_cell); fr(m->dz_tc); fr(m->disc_dpre); fr(m->disc_db);
  fr(m->noise_eps); fr(m->latbuf); fr(m->dlat); fr(m->z); fr(m->sig); fr(m->eps); fr(m->kl);
  fr(m->latlbuf); fr(m->dlatl); fr(m->lsmp); fr(m->lsig); fr(m->leps); fr(m->kl_l); fr(m->dl);
  fr(m->P); fr(m->dP); fr(m->raw); fr(m->draw); fr(m->rho); fr(m->llk_part); fr(m->llk_y); fr(m->llk_o); fr(m->slab);
  fr(m->chunks); fr(m->partial); fr(m->shard_partial); fr(m->tensor_norm); fr(m->sq_slots);
  if (m->pinned) hipHostFree(m->pinned);
  if (m->order_pin) hipHostFree(m->order_pin);
  if (m->metrics_pin) hipHostFree(m->metrics_pin);
  if (m->seam_state) hipFree(m->seam_state);
  if (m->score_pin) hipHostFree(m->score_pin);
  if (m->ev_order) hipEventDestroy(m->ev_order);
  if (m->pred_stage) hipFree(m->pred_stage);
  if (m->pred_target) hipFree(m->pred_target);
  if (m->csr_host) hipFree(m->csr_host);
  if (m->pred_ids) hipFree(m->pred_ids);
  if (m->imp_d) hipFree(m->imp_d);
  if (m->imp_hist) hipFree(m->imp_hist);
  if (m->pred_sel) hipFree(m->pred_sel);
  if (m->cor_keep) hipFree(m->cor_keep);
  if (m->cor_ops) hipFree(m->cor_ops);
  if (m->score_buf) hipFree(m->score_buf);
  if (m->score_wimg) hipFree(m->score_wimg);
  if (m->score_aux) hipFree(m->score_aux);
  for (auto& kv : m->injected) fr(kv.second.d);
  if (m->st_comm) { hipStreamSynchronize(m->st_comm); hipStreamDestroy(m->st_comm); }
  if (m->st_side) { hipStreamSynchronize(m->st_side); hipStreamDestroy(m->st_side); }
  if (m->ev_hf) hipEventDestroy(m->ev_hf);
  if (m->ev_sweep) hipEventDestroy(m->ev_sweep);
  if (m->ev_c1) hipEventDestroy(m->ev_c1);
  if (m->ev_c2) hipEventDestroy(m->ev_c2);
  if (m->ev_c3) hipEventDestroy(m->ev_c3);
  if (m->st) hipStreamDestroy(m->st);
  delete m;
  return SMX_OK;
}

int smx_num_tensors(const smx_model* m) { return m ? (int)m->tensors.size() : 0; }

int smx_tensor_info(const smx_model* m, int index, char* name, int name_cap, int32_t* rows, int32_t* cols) {
  SMX_REQUIRE(m && index >= 0 && index < (int)m->tensors.size(), "tensor index out of range");
  const TensorInfo& t = m->tensors[index];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (rows) *rows = t.rows;
  if (cols) *cols = t.cols;
  return SMX_OK;
}

static float* which_buf(smx_model* m, int which) {
  switch (which) { case 0: return m->params; case 1: return m->grads; case 2: return m->adam_m; case 3: return m->adam_v; }
  return nullptr;
}

int smx_get_tensor(smx_model* m, int which, int index, float* host) {
  SMX_REQUIRE(m && host && index >= 0 && index < (int)m->tensors.size(), "bad tensor index");
  float* base = which_buf(m, which);
  SMX_REQUIRE(base, "which must be 0..3");
  const TensorInfo& t = m->tensors[index];
  SMX_REQUIRE(!(m->opt_stale && (which == 2 || which == 3) && t.offset >= m->bucket1_off),
              "the heads' Adam moments are sharded over the ranks (flag opt_shard): call smx_opt_gather on every rank first");
  std::vector<float> dev(t.count);
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(dev.data(), base + t.offset, t.count * sizeof(float), hipMemcpyDeviceToHost));
  unpack(t, dev, host, 1.f);
  return SMX_OK;
}

int smx_set_tensor(smx_model* m, int which, int index, const float* host) {
  SMX_REQUIRE(m && host && index >= 0 && index < (int)m->tensors.size(), "bad tensor index");
  float* base = which_buf(m, which);
  SMX_REQUIRE(base, "which must be 0..3");
  const TensorInfo& t = m->tensors[index];
  std::vector<float> dev;
  pack(t, host, dev);
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(base + t.offset, dev.data(), t.count * sizeof(float), hipMemcpyHostToDevice));
  if (which == 0) ++m->params_epoch;
  return SMX_OK;
}

// ---- padding audit (test instrument: the invariant of smx_model.h's layout note, read back from the device) ----------------------
namespace smx {
// one work buffer as the audit walks it.  form 0: f32 [rows][ld], padding = columns >= width; 1: f32 k-major [wp][ld] (ld >= rows),
// padding = rows of it >= width; 2: the three-way bf16 split [3][rows][wp], padding = columns >= width
struct AuditBuf { std::string name; const void* p = nullptr; long rows = 0; int ld = 0, width = 0, wp = 0, form = 0; };
static inline bool pad_nonzero(float v) { uint32_t b; memcpy(&b, &v, 4); return (b & 0x7fffffffu) != 0u; }
// whether element i of tensor t's [offset, offset + count) lies outside the logical extent (rows < rows, columns < chunk_w of their chunk)
static inline bool pad_element(const TensorInfo& t, size_t i) {
  const size_t r = i / (size_t)t.ld, c = i % (size_t)t.ld;
  return (int)r >= t.rows || (int)(c % (size_t)t.chunk_wp) >= t.chunk_w;
}
struct PadTally {
  int64_t n_bad = 0, first_offset = -1; int first = -1; std::string first_name;
  void hit(int index, const std::string& name, int64_t off) {
    if (n_bad++ == 0) { first = index; first_name = name; first_offset = off; }
  }
};
// one work buffer of the last pass (AuditBuf): its padding alone copied to the host, walked there
static int pad_audit_buf(const AuditBuf& b, int index, PadTally& tl) {
  if (!b.p || b.rows <= 0 || b.wp <= b.width) return SMX_OK;
  const size_t pw = (size_t)(b.wp - b.width);
  if (b.form == 2) {   // three images [rows][wp] of bf16, one behind the other: 3 x rows rows of wp
    const size_t nr = (size_t)3 * b.rows;
    std::vector<uint16_t> h(nr * pw);
    SMX_HIP(hipMemcpy2D(h.data(), pw * 2, static_cast<const uint16_t*>(b.p) + b.width, (size_t)b.wp * 2, pw * 2, nr, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i)
      if (h[i] & 0x7fffu) tl.hit(index, b.name, (int64_t)((i / pw) * b.wp + b.width + i % pw));
    return SMX_OK;
  }
  const float* src = static_cast<const float*>(b.p);
  if (b.form == 1) {   // k-major [wp][ld]: rows width .. wp - 1 of it, the first `rows` entries of each
    std::vector<float> h(pw * (size_t)b.rows);
    SMX_HIP(hipMemcpy2D(h.data(), (size_t)b.rows * 4, src + (size_t)b.width * b.ld, (size_t)b.ld * 4, (size_t)b.rows * 4, pw, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i)
      if (pad_nonzero(h[i])) tl.hit(index, b.name, (int64_t)((b.width + i / b.rows) * b.ld + i % b.rows));
    return SMX_OK;
  }
  std::vector<float> h((size_t)b.rows * pw);
  SMX_HIP(hipMemcpy2D(h.data(), pw * 4, src + b.width, (size_t)b.ld * 4, pw * 4, (size_t)b.rows, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < h.size(); ++i)
    if (pad_nonzero(h[i])) tl.hit(index, b.name, (int64_t)((i / pw) * b.ld + b.width + i % pw));
  return SMX_OK;
}
// the work buffers smx_pad_audit(which = 4) covers, as the last pass left them
static std::vector<AuditBuf> pad_work_buffers(smx_model* m) {
  std::vector<AuditBuf> v;
  auto add = [&](const std::string& name, const float* p, long rows, int ld, int width, int wp, int col0 = 0) {
    AuditBuf b;
    b.name = name; b.p = p ? p + col0 : nullptr; b.rows = rows; b.ld = ld; b.width = width; b.wp = wp;
    v.push_back(b);
  };
  const long R = std::min(m->audit_rows, m->Rmax);
  const char* const pre[3] = {"enc", "encl", "dec"};
  int n = 0;
  for (auto* mlp : {&m->enc, &m->encl, &m->dec}) {
    for (size_t i = 0; i < mlp->size(); ++i) add(std::string(pre[n]) + std::to_string(i) + " out", (*mlp)[i].out_buf, R, (*mlp)[i].out_p, (*mlp)[i].out, (*mlp)[i].out_p);
    ++n;
  }
  const long R2 = std::min(m->audit_disc_rows, 2 * m->Bmax);
  for (size_t i = 0; i < m->disc.size(); ++i) add("disc" + std::to_string(i) + " out", m->disc[i].out_buf, R2, m->disc[i].out_p, m->disc[i].out, m->disc[i].out_p);
  add("z", m->z, R, m->Dp, m->D, m->Dp);
  if (m->scvi) add("library latent head", m->latlbuf, R, 32, 2, 32);
  for (int c = 0; c < m->k; ++c) add("dP plane " + std::to_string(c), m->dP, R, m->k * m->Gp, m->G, m->Gp, c * m->Gp);
  // the stacked evaluation decoder's buffers, from score_buf's layout as its callers cut it (smx_scoring.hip / smx_predict.hip): the two
  // alternating buffers hold the last two layers' outputs; a scoring call's last layer also stands k-major or bf16-split behind them
  const AuditStacked& sk = m->audit_stk;
  int Hmax = 0;
  for (const MlpLayer& L : m->dec) Hmax = std::max(Hmax, L.out_p);
  const size_t need = sk.form < 0 ? 0 : (size_t)sk.cap * ((size_t)m->Dp + 1 + (size_t)(sk.form == 0 ? 2 : 4) * Hmax);
  if (sk.form >= 0 && m->score_buf && sk.rows <= sk.cap && need <= m->score_floats) {   // (a scratch regrown smaller since: nothing of it is left)
    float* hb[2] = {m->score_buf + (size_t)sk.cap * (m->Dp + 1), m->score_buf + (size_t)sk.cap * (m->Dp + 1 + Hmax)};
    const float* ht = hb[1] + (size_t)sk.cap * Hmax;
    const size_t n = m->dec.size();
    for (size_t i = n >= 2 ? n - 2 : 0; i < n && sk.form != 3; ++i)
      add("stacked dec" + std::to_string(i), hb[i & 1], sk.rows, m->dec[i].out_p, m->dec[i].out, m->dec[i].out_p);
    if (sk.form >= 1) {
      const MlpLayer& L = m->dec.back();
      AuditBuf b;
      b.name = std::string("stacked dec") + std::to_string(n - 1) + (sk.form == 1 ? " (k-major)" : " (bf16 split)");
      b.p = ht; b.rows = sk.rows; b.width = L.out; b.wp = L.out_p; b.form = sk.form == 1 ? 1 : 2; b.ld = sk.form == 1 ? (int)sk.rows : L.out_p;
      v.push_back(b);
    }
  }
  return v;
}
}  // namespace smx

int smx_pad_audit(smx_model* m, int32_t which, int64_t* n_bad, int32_t* first_tensor, int64_t* first_offset, char* first_name, int32_t name_cap) {
  SMX_REQUIRE(m && n_bad, "null argument");
  SMX_REQUIRE(which >= 0 && which <= 4, "which must be 0..4");
  SMX_REQUIRE(!(m->opt_stale && (which == 2 || which == 3)),
              "the heads' Adam moments are sharded over the ranks (flag opt_shard): call smx_opt_gather on every rank first");
  SMX_CHECK(head_sweep_join(m));   // (the heads' background update, if one is under way on the second stream)
  SMX_HIP(hipStreamSynchronize(m->st));
  PadTally tl;
  if (which == 4) {
    const std::vector<AuditBuf> bufs = pad_work_buffers(m);
    for (size_t i = 0; i < bufs.size(); ++i) SMX_CHECK(pad_audit_buf(bufs[i], (int)i, tl));
  } else {
    std::vector<float> h(m->flat_count);
    SMX_HIP(hipMemcpy(h.data(), which_buf(m, which), h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < m->tensors.size(); ++t) {
      const TensorInfo& ti = m->tensors[t];
      for (size_t i = 0; i < ti.count; ++i)
        if (pad_element(ti, i) && pad_nonzero(h[ti.offset + i])) tl.hit((int)t, ti.name, (int64_t)i);
    }
  }
  *n_bad = tl.n_bad;
  if (first_tensor) *first_tensor = tl.first;
  if (first_offset) *first_offset = tl.first_offset;
  if (first_name && name_cap > 0) { strncpy(first_name, tl.first_name.c_str(), name_cap - 1); first_name[name_cap - 1] = 0; }
  return SMX_OK;
}

int smx_pad_poke(smx_model* m, int32_t which, int32_t index, float value) {
  SMX_REQUIRE(m && index >= 0 && index < (int)m->tensors.size(), "bad tensor index");
  float* base = which_buf(m, which);
  SMX_REQUIRE(base, "which must be 0..3");
  const TensorInfo& t = m->tensors[index];
  size_t at = t.count;
  for (size_t i = 0; i < t.count; ++i) if (pad_element(t, i)) { at = i; break; }
  SMX_REQUIRE(at < t.count, "smx_pad_poke: the tensor has no padding");
  SMX_REQUIRE(!(m->opt_stale && (which == 2 || which == 3) && t.offset >= m->bucket1_off),
              "the heads' Adam moments are sharded over the ranks (flag opt_shard): call smx_opt_gather on every rank first");
  SMX_CHECK(head_sweep_join(m));
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(base + t.offset + at, &value, sizeof(float), hipMemcpyHostToDevice));
  if (which == 0) ++m->params_epoch;
  return SMX_OK;
}

int smx_num_bn_layers(const smx_model* m) { return m ? (int)m->bn_w.size() : 0; }

int smx_get_bn(smx_model* m, int layer, int which, float* host, int32_t* width) {
  SMX_REQUIRE(m && layer >= 0 && layer < (int)m->bn_w.size() && (which == 0 || which == 1), "bad bn layer");
  if (width) *width = m->bn_w[layer];
  if (host) {
    SMX_HIP(hipStreamSynchronize(m->st));
    SMX_HIP(hipMemcpy(host, m->bn_moving + m->bn_off[layer] + (size_t)which * m->bn_wp[layer],
                      m->bn_w[layer] * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SMX_OK;
}

int smx_set_bn(smx_model* m, int layer, int which, const float* host) {
  SMX_REQUIRE(m && host && layer >= 0 && layer < (int)m->bn_w.size() && (which == 0 || which == 1), "bad bn layer");
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(m->bn_moving + m->bn_off[layer] + (size_t)which * m->bn_wp[layer], host,
                    m->bn_w[layer] * sizeof(float), hipMemcpyHostToDevice));
  return SMX_OK;
}

int smx_get_step(const smx_model* m, int32_t* step) {
  SMX_REQUIRE(m && step, "null argument");
  *step = (int32_t)m->h_next;
  return SMX_OK;
}

int smx_set_step(smx_model* m, int32_t step) {
  SMX_REQUIRE(m && step >= 0, "bad step");
  StepState s[3];
  memset(s, 0, sizeof(s));
  s[2].next = (uint32_t)step;
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemcpy(m->state3, s, sizeof(s), hipMemcpyHostToDevice));
  m->h_next = (uint32_t)step;
  return SMX_OK;
}

int smx_set_noise(smx_model* m, int32_t stream, const float* data, int32_t batch, int32_t width) {
  SMX_REQUIRE(m && data && batch > 0 && batch <= m->Bmax && width > 0, "bad noise block");
  const int ld = round_up(width, 32);
  Injected& ij = m->injected[stream];
  if (ij.d && ij.ld != ld) { hipFree(ij.d); ij.d = nullptr; }
  if (!ij.d) { SMX_CHECK(dmalloc(&ij.d, (size_t)m->Bmax * ld)); ij.ld = ld; }
  SMX_HIP(hipStreamSynchronize(m->st));
  SMX_HIP(hipMemset(ij.d, 0, (size_t)m->Bmax * ld * sizeof(float)));
  SMX_HIP(hipMemcpy2D(ij.d, (size_t)ld * sizeof(float), data, (size_t)width * sizeof(float), (size_t)width * sizeof(float),
                      (size_t)batch, hipMemcpyHostToDevice));
  m->use_injected = true;
  return SMX_OK;
}

int smx_clear_noise(smx_model* m) {
  SMX_REQUIRE(m, "null model");
  SMX_HIP(hipStreamSynchronize(m->st));
  for (auto& kv : m->injected) if (kv.second.d) hipFree(kv.second.d);
  m->injected.clear();
  m->use_injected = false;
  return SMX_OK;
}

int smx_set_flag(smx_model* m, const char* name, int value) {
  SMX_REQUIRE(m && name, "null argument");
  SMX_HIP(hipStreamSynchronize(m->st));
  const std::string n(name);
  int* f = n == "head_loss" ? &m->flags.head_loss : n == "head_fused" ? &m->flags.head_fused : n == "head_sweep" ? &m->flags.head_sweep : n == "front" ? &m->flags.front : n == "bwd_front" ? &m->flags.bwd_front
         : n == "head_bwd" ? &m->flags.head_bwd : n == "wgrad" ? &m->flags.wgrad : n == "scvi_fused" ? &m->flags.scvi_fused
         : n == "twin" ? &m->flags.twin : n == "label_ride" ? &m->flags.label_ride : n == "act_epilogue" ? &m->flags.act_epilogue
         : n == "stacked_scoring" ? &m->flags.stacked_scoring : n == "bf16x3" ? &m->flags.bf16x3 : n == "opt_shard" ? &m->flags.opt_shard
         : n == "tie_mixtures" ? &m->flags.tie_mixtures : n == "tie_loc" ? &m->flags.tie_loc : n == "tie_scale" ? &m->flags.tie_scale : nullptr;
  SMX_REQUIRE(f, "unknown flag (head_loss, head_fused, head_sweep, front, bwd_front, head_bwd, wgrad, scvi_fused, twin, label_ride, act_epilogue, stacked_scoring, bf16x3, opt_shard; SCALE: tie_mixtures, tie_loc, tie_scale)");
  *f = (f == &m->flags.bf16x3 && value < 0) ? -1 : (value ? 1 : 0);   // bf16x3: -1 = by the width of the head (the default)
  drop_graphs(m);   // a captured step bakes the launch sequence in
  return SMX_OK;
}

int smx_set_activation(smx_model* m, int32_t net, int32_t act) {
  SMX_REQUIRE(m, "null model");
  SMX_REQUIRE(act >= SMX_ACT_RELU && act <= SMX_ACT_SOFTPLUS, "smx_set_activation: unknown activation");
  std::vector<MlpLayer>* mlp = net == SMX_NET_ENCODER ? &m->enc : net == SMX_NET_DECODER ? &m->dec : net == SMX_NET_LIBRARY_ENCODER ? &m->encl : nullptr;
  SMX_REQUIRE(mlp, "smx_set_activation: unknown network (encoder 0, decoder 1, library encoder 2)");
  SMX_REQUIRE(net != SMX_NET_LIBRARY_ENCODER || !m->encl.empty(), "smx_set_activation: the model has no library encoder");
  SMX_HIP(hipStreamSynchronize(m->st));
  for (auto& L : *mlp) L.act = act;
  drop_graphs(m);   // a captured step bakes the launch forms in
  return SMX_OK;
}

int smx_timing_enable(smx_model* m, const char* kernel) {
  SMX_REQUIRE(m, "null model");
  SMX_HIP(hipStreamSynchronize(m->st));
  m->timing_label = kernel ? kernel : "";
  m->timing_reps = SMX_LOSS_TIMING_REPEAT;
  // "label@N": the idempotent likelihood kernels are launched N times per event pair instead of the default 8
  // (N = 1: one launch inside the pair, the figure rocprofv3's per-kernel duration is compared with)
  const size_t at = m->timing_label.find('@');
  if (at != std::string::npos) {
    m->timing_reps = std::max(1, atoi(m->timing_label.c_str() + at + 1));
    m->timing_label.resize(at);
  }
  m->timing_used = 0;
  return SMX_OK;
}

int smx_timing_read(smx_model* m, double* total_ms, int64_t* launches) {
  SMX_REQUIRE(m && total_ms && launches, "null argument");
  SMX_HIP(hipStreamSynchronize(m->st));
  double tot = 0.0;
  for (size_t i = 0; i < m->timing_used; ++i) {
    float ms = 0.f;
    SMX_HIP(hipEventElapsedTime(&ms, m->timing_events[i].first, m->timing_events[i].second));
    tot += ms;
  }
  *total_ms = tot; *launches = (int64_t)m->timing_used;
  m->timing_used = 0;
  return SMX_OK;
}

int64_t smx_loss_bytes_per_cell(const smx_model* m) {
  if (!m) return 0;
  return (int64_t)(4 + 8 * m->k) * m->G + 16 * (int64_t)m->D + 4;
}

// (forward_pass's own predicate, smx_forward.hip: head_fused_ok)
int64_t smx_head_fused_bytes(const smx_model* m, int32_t batch) {
  if (!m || batch <= 0 || m->dec.empty()) return 0;
  return head_fused_ok(m, batch) ? (int64_t)head_fused_bytes(batch, m->G, m->Gp, m->k) : 0;
}

int32_t smx_head_dw_late(const smx_model* m) { return (m && m->dw_late_now) ? 1 : 0; }   // (smx_backward.hip: dw_late)
int32_t smx_lazy_adam_steps(const smx_model* m) { return m ? m->lazy_steps : 0; }          // (smx_step.hip: the lazy encoder update)
int32_t smx_bwd_seam_steps(const smx_model* m) { return m ? m->seam_steps : 0; }            // (smx_backward.hip: the seam form)

}  // extern "C"
