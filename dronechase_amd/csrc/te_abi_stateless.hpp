// te_abi_stateless.hpp — every C ABI entry that takes no te_env (included by te_env.hip at the end of its extern "C" region): the
// policy's shapes, packing, te_policy_act*, te_policy_ppo_grad* and optimiser step, the level5 student's sphere encoder, advantage
// estimation, te_policy_ppo_epoch, the episode monitor and the imitation dataset.  Every check is on the host, before any launch;
// launches go through te_host.hpp's stateless_launch, the policy's with te_policy_host.hpp's tables and geometry.  te_drive_wingman*,
// which takes a te_env, is te_env.hip's.
#pragma once

static int policy_words(int32_t lidar_channels, size_t* out) {
  if (lidar_channels != 2 && lidar_channels != 3) return fail("te_policy: lidar_channels must be 2 or 3");
  *out = (size_t)policy_layout(pol_shape(POL_SHAPE_DEFAULT, lidar_channels)).words;
  return 0;
}

__attribute__((visibility("default"))) int te_policy_shape_check(const te_policy_shape* shape) {
  return policy_shape_id(shape, "te_policy_shape_check") < 0;
}

__attribute__((visibility("default"))) int te_policy_param_words_shaped(const te_policy_shape* shape, size_t* out_words) {
  return policy_shaped_words("te_policy_param_words_shaped", shape, out_words, policy_layout);
}

__attribute__((visibility("default"))) int te_policy_param_words(int32_t lidar_channels, size_t* out_words) {
  if (!out_words) return fail("te_policy_param_words: null argument");
  return policy_words(lidar_channels, out_words);
}

__attribute__((visibility("default"))) int te_policy_bf16_words(const te_policy_shape* shape, size_t* out_halfwords) {
  return policy_shaped_words("te_policy_bf16_words", shape, out_halfwords, policy_bf16_layout);
}

__attribute__((visibility("default"))) int te_policy_pack_bf16(const float* params, const te_policy_shape* shape, uint16_t* out, void* stream) {
  return policy_pack("te_policy_pack_bf16", params, shape, out, stream, policy_pack_plan, policy_pack_bf16_kernel);
}

// The three act entries behind their shape checks (fn: the caller's name in the messages).  bf16: te_policy_act_bf16, which also takes
// weights_bf16 and launches the bf16 instance on its own LDS plan
static int policy_act(const char* fn, bool bf16, int shape_id, const float* params, const uint16_t* weights_bf16, int32_t lidar_channels, int32_t n,
                      const float* lidar, const float* inertial, const float* last_action, const float* eps, float* mu, float* value, float* action,
                      float* logp, float* action_env, void* stream) {
  const std::string who = std::string(fn);
  if (n <= 0) return fail(who + ": n must be positive");
  if (!params || (bf16 && !weights_bf16) || !lidar || !inertial || !last_action || !mu || !value) return fail(who + ": null argument");
  if (eps && (!action || !logp || !action_env)) return fail(who + ": eps given, so action, logp and action_env must be too");
  if ((uintptr_t)params & 15) return fail(who + ": params must be 16-byte aligned");
  if (bf16 && ((uintptr_t)weights_bf16 & 15)) return fail(who + ": weights_bf16 must be 16-byte aligned");
  if ((uintptr_t)lidar & 7) return fail(who + ": lidar must be 8-byte aligned");
  for (const void* q : {(const void*)inertial, (const void*)last_action, (const void*)eps, (const void*)mu, (const void*)value,
                        (const void*)action, (const void*)logp, (const void*)action_env})
    if ((uintptr_t)q & 3) return fail(who + ": float arrays must be 4-byte aligned");
  const PolicyIO io{lidar, inertial, last_action, eps, mu, value, eps ? action : nullptr, eps ? logp : nullptr, eps ? action_env : nullptr, n};
  const PolShape shape = pol_shape(shape_id, lidar_channels);
  const PolicyParams P = policy_params(shape, params);
  const PolGeom g = bf16 ? pol_geom(pol_lds_plan_bf16(shape)) : pol_geom(pol_lds_plan(shape));
  if (bf16)
    return stateless_launch(kPolicyActBf16Kernels[shape_id][lidar_channels - 2], g.groups(n), g.threads, g.lds_bytes, stream, P,
                            policy_weights(shape, weights_bf16), io);
  return stateless_launch(kPolicyActKernels[shape_id][lidar_channels - 2], g.groups(n), g.threads, g.lds_bytes, stream, P, io);
}

__attribute__((visibility("default"))) int te_policy_act(const float* params, int32_t lidar_channels, int32_t n, const float* lidar,
                                                         const float* inertial, const float* last_action, const float* eps, float* mu,
                                                         float* value, float* action, float* logp, float* action_env, void* stream) {
  size_t words;
  if (policy_words(lidar_channels, &words)) return 1;
  return policy_act("te_policy_act", false, POL_SHAPE_DEFAULT, params, nullptr, lidar_channels, n, lidar, inertial, last_action, eps, mu, value,
                    action, logp, action_env, stream);
}

__attribute__((visibility("default"))) int te_policy_act_shaped(const float* params, const te_policy_shape* shape, int32_t n, const float* lidar,
                                                                const float* inertial, const float* last_action, const float* eps, float* mu,
                                                                float* value, float* action, float* logp, float* action_env, void* stream) {
  const int id = policy_shape_id(shape, "te_policy_act_shaped");
  if (id < 0) return 1;
  return policy_act("te_policy_act_shaped", false, id, params, nullptr, shape->lidar_channels, n, lidar, inertial, last_action, eps, mu, value,
                    action, logp, action_env, stream);
}

__attribute__((visibility("default"))) int te_policy_act_bf16(const float* params, const uint16_t* weights_bf16, const te_policy_shape* shape,
                                                              int32_t n, const float* lidar, const float* inertial, const float* last_action,
                                                              const float* eps, float* mu, float* value, float* action, float* logp,
                                                              float* action_env, void* stream) {
  const int id = policy_shape_id(shape, "te_policy_act_bf16");
  if (id < 0) return 1;
  return policy_act("te_policy_act_bf16", true, id, params, weights_bf16, shape->lidar_channels, n, lidar, inertial, last_action, eps, mu, value,
                    action, logp, action_env, stream);
}

// The gradient entries behind their shape checks (fn: the caller's name in the messages; size_fn: the entry that tells the workspace's
// size; bf16: te_policy_ppo_grad_bf16's workspace and kernels, te_policy_grad_bf16.hpp).  n up to 2^27: the conv1 layer's 12 * n
// reduction rows stay within int
static int policy_grad_rows_check(const std::string& who, int32_t n) {
  if (n <= 0) return fail(who + ": n must be positive");
  if (n > (1 << 27)) return fail(who + ": n must be at most 2^27");
  return 0;
}

static int policy_grad_workspace(const char* fn, bool bf16, int shape_id, int32_t lidar_channels, int32_t n, size_t* out_bytes) {
  if (policy_grad_rows_check(fn, n)) return 1;
  const PolShape shape = pol_shape(shape_id, lidar_channels);
  *out_bytes = bf16 ? policy_grad_bf16_layout(shape, n, nullptr, policy_layout(shape), nullptr, nullptr, nullptr, nullptr)
                    : policy_grad_layout(shape, n, nullptr, policy_layout(shape), nullptr, nullptr, nullptr, nullptr);
  return 0;
}

// One gradient call's arguments but the rows: what te_policy_ppo_epoch keeps from minibatch to minibatch
struct PolGradCall {
  bool bf16;
  int shape_id;
  const float* params;
  const uint16_t *weights_bf16, *weights_bf16_t;
  int32_t lidar_channels;
  const float *lidar, *inertial, *last_action;
  PolLossInputs loss;
  float *grad, *stats;
  void* workspace;
  size_t workspace_bytes;
};

// every check of a gradient call over the n rows `index`, on the host: nothing is launched
static int policy_ppo_grad_check(const std::string& who, const char* size_fn, const PolGradCall& c, int32_t n, const int64_t* index) {
  const PolLossInputs& loss = c.loss;
  if (policy_grad_rows_check(who, n)) return 1;
  if (!c.params || (c.bf16 && (!c.weights_bf16 || !c.weights_bf16_t)) || !c.lidar || !c.inertial || !c.last_action || !loss.action || !loss.old_logp ||
      !loss.adv || !loss.ret || !c.grad || !c.stats || !c.workspace)
    return fail(who + ": null argument");
  if ((uintptr_t)c.params & 15) return fail(who + ": params must be 16-byte aligned");
  if (c.bf16 && ((uintptr_t)c.weights_bf16 & 15)) return fail(who + ": weights_bf16 must be 16-byte aligned");
  if (c.bf16 && ((uintptr_t)c.weights_bf16_t & 15)) return fail(who + ": weights_bf16_t must be 16-byte aligned");
  if ((uintptr_t)c.grad & 15) return fail(who + ": grad must be 16-byte aligned");
  if ((uintptr_t)c.lidar & 7) return fail(who + ": lidar must be 8-byte aligned");
  if ((uintptr_t)c.workspace & 255) return fail(who + ": workspace must be 256-byte aligned");
  if ((uintptr_t)index & 7) return fail(who + ": index must be 8-byte aligned");
  for (const void* q : {(const void*)c.inertial, (const void*)c.last_action, (const void*)loss.action, (const void*)loss.old_logp,
                        (const void*)loss.adv, (const void*)loss.ret, (const void*)loss.adv_mean_std, (const void*)c.stats})
    if ((uintptr_t)q & 3) return fail(who + ": float arrays must be 4-byte aligned");
  size_t need = 0;
  if (policy_grad_workspace(who.c_str(), c.bf16, c.shape_id, c.lidar_channels, n, &need)) return 1;
  if (c.workspace_bytes < need)
    return fail(who + ": workspace too small (" + std::to_string(c.workspace_bytes) + " bytes, " + size_fn + " says " + std::to_string(need) + ")");
  if (!std::isfinite(loss.clip_range) || loss.clip_range < 0.f) return fail(who + ": clip_range must be finite and >= 0");
  return 0;
}

// the three launches of a checked gradient call
static int policy_ppo_grad_launch(const PolGradCall& c, int32_t n, const int64_t* index, void* stream) {
  GradTileArgs t; GradTileArgsB tb; GradPlan g;
  const PolShape shape = pol_shape(c.shape_id, c.lidar_channels);
  const PolicyParams P = policy_params(shape, c.params);
  char* const ws = static_cast<char*>(c.workspace);
  if (c.bf16) policy_grad_bf16_layout(shape, n, ws, P, c.grad, c.stats, &tb, &g);
  else policy_grad_layout(shape, n, ws, P, c.grad, c.stats, &t, &g);
  const PolicyIn in{c.lidar, c.inertial, c.last_action, index, n};
  // the tile grid covers the workspace's Bp rows (n rounded up to 32), not n: a 16-row shape's padding tile writes its rows too, and a
  // padding row writes its zeros like any other
  const int Bp = g.L[POL_L_MU].R;
  const PolGeom tile = c.bf16 ? pol_geom(pol_grad_lds_plan_bf16(shape)) : pol_geom(pol_lds_plan(shape));
  if (c.bf16) {
    policy_loss_inputs(tb, c.loss, n);
    if (stateless_launch(kPolicyGradBf16Kernels[c.shape_id][c.lidar_channels - 2], tile.groups(Bp), tile.threads, tile.lds_bytes, stream, P,
                         policy_weights(shape, c.weights_bf16), policy_weights_t(shape, c.weights_bf16_t), in, tb))
      return 1;
  } else {
    policy_loss_inputs(t, c.loss, n);
    if (stateless_launch(kPolicyGradKernels[c.shape_id][c.lidar_channels - 2], tile.groups(Bp), tile.threads, tile.lds_bytes, stream, P, in, t))
      return 1;
  }
  if (stateless_launch(c.bf16 ? policy_wgrad_bf16_kernel : policy_wgrad_kernel, g.wgs, 256, 0, stream, g)) return 1;
  return stateless_launch(policy_grad_combine_kernel, (g.words + 255) / 256, 256, 0, stream, g);
}

static int policy_ppo_grad(const char* fn, const char* size_fn, bool bf16, int shape_id, const float* params, const uint16_t* weights_bf16,
                           const uint16_t* weights_bf16_t, int32_t lidar_channels, int32_t n, const int64_t* index, const float* lidar,
                           const float* inertial, const float* last_action, const PolLossInputs& loss, float* grad, float* stats, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const PolGradCall c{bf16, shape_id, params, weights_bf16, weights_bf16_t, lidar_channels, lidar, inertial, last_action, loss, grad, stats,
                      workspace, workspace_bytes};
  if (policy_ppo_grad_check(fn, size_fn, c, n, index)) return 1;
  return policy_ppo_grad_launch(c, n, index, stream);
}

__attribute__((visibility("default"))) int te_policy_grad_workspace_bytes(int32_t lidar_channels, int32_t n, size_t* out_bytes) {
  size_t words;
  if (!out_bytes) return fail("te_policy_grad_workspace_bytes: null argument");
  if (policy_words(lidar_channels, &words)) return 1;
  return policy_grad_workspace("te_policy_grad_workspace_bytes", false, POL_SHAPE_DEFAULT, lidar_channels, n, out_bytes);
}

// te_policy_grad_workspace_bytes_shaped (bf16 false) and te_policy_grad_bf16_workspace_bytes (true)
static int policy_grad_workspace_shaped(const char* fn, bool bf16, const te_policy_shape* shape, int32_t n, size_t* out_bytes) {
  if (!out_bytes) return fail(std::string(fn) + ": null argument");
  const int id = policy_shape_id(shape, fn);
  if (id < 0) return 1;
  return policy_grad_workspace(fn, bf16, id, shape->lidar_channels, n, out_bytes);
}

__attribute__((visibility("default"))) int te_policy_grad_workspace_bytes_shaped(const te_policy_shape* shape, int32_t n, size_t* out_bytes) {
  return policy_grad_workspace_shaped("te_policy_grad_workspace_bytes_shaped", false, shape, n, out_bytes);
}

__attribute__((visibility("default"))) int te_policy_ppo_grad(const float* params, int32_t lidar_channels, int32_t n, const int64_t* index,
                                                              const float* lidar, const float* inertial, const float* last_action,
                                                              const float* action, const float* old_logp, const float* adv, const float* ret,
                                                              const float* adv_mean_std, float clip_range, float vf_coef, float ent_coef,
                                                              float* grad, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  size_t words;
  if (policy_words(lidar_channels, &words)) return 1;
  return policy_ppo_grad("te_policy_ppo_grad", "te_policy_grad_workspace_bytes", false, POL_SHAPE_DEFAULT, params, nullptr, nullptr, lidar_channels,
                         n, index, lidar, inertial, last_action, {action, old_logp, adv, ret, adv_mean_std, clip_range, vf_coef, ent_coef}, grad,
                         stats, workspace, workspace_bytes, stream);
}

__attribute__((visibility("default"))) int te_policy_ppo_grad_shaped(const float* params, const te_policy_shape* shape, int32_t n,
                                                                     const int64_t* index, const float* lidar, const float* inertial,
                                                                     const float* last_action, const float* action, const float* old_logp,
                                                                     const float* adv, const float* ret, const float* adv_mean_std,
                                                                     float clip_range, float vf_coef, float ent_coef, float* grad, float* stats,
                                                                     void* workspace, size_t workspace_bytes, void* stream) {
  const int id = policy_shape_id(shape, "te_policy_ppo_grad_shaped");
  if (id < 0) return 1;
  return policy_ppo_grad("te_policy_ppo_grad_shaped", "te_policy_grad_workspace_bytes_shaped", false, id, params, nullptr, nullptr,
                         shape->lidar_channels, n, index, lidar, inertial, last_action,
                         {action, old_logp, adv, ret, adv_mean_std, clip_range, vf_coef, ent_coef}, grad, stats, workspace, workspace_bytes, stream);
}

// ---- te_policy_ppo_grad_bf16 (te_policy_grad_bf16.hpp)
__attribute__((visibility("default"))) int te_policy_bf16_grad_words(const te_policy_shape* shape, size_t* out_halfwords) {
  return policy_shaped_words("te_policy_bf16_grad_words", shape, out_halfwords, policy_bf16_t_layout);
}

__attribute__((visibility("default"))) int te_policy_pack_bf16_grad(const float* params, const te_policy_shape* shape, uint16_t* out, void* stream) {
  return policy_pack("te_policy_pack_bf16_grad", params, shape, out, stream, policy_pack_t_plan, policy_pack_bf16_t_kernel);
}

__attribute__((visibility("default"))) int te_policy_grad_bf16_workspace_bytes(const te_policy_shape* shape, int32_t n, size_t* out_bytes) {
  return policy_grad_workspace_shaped("te_policy_grad_bf16_workspace_bytes", true, shape, n, out_bytes);
}

__attribute__((visibility("default"))) int te_policy_ppo_grad_bf16(const float* params, const uint16_t* weights_bf16, const uint16_t* weights_bf16_t,
                                                                   const te_policy_shape* shape, int32_t n, const int64_t* index,
                                                                   const float* lidar, const float* inertial, const float* last_action,
                                                                   const float* action, const float* old_logp, const float* adv, const float* ret,
                                                                   const float* adv_mean_std, float clip_range, float vf_coef, float ent_coef,
                                                                   float* grad, float* stats, void* workspace, size_t workspace_bytes,
                                                                   void* stream) {
  const int id = policy_shape_id(shape, "te_policy_ppo_grad_bf16");
  if (id < 0) return 1;
  return policy_ppo_grad("te_policy_ppo_grad_bf16", "te_policy_grad_bf16_workspace_bytes", true, id, params, weights_bf16, weights_bf16_t,
                         shape->lidar_channels, n, index, lidar, inertial, last_action,
                         {action, old_logp, adv, ret, adv_mean_std, clip_range, vf_coef, ent_coef}, grad, stats, workspace, workspace_bytes, stream);
}

// ---- optimiser step (te_policy_opt.hpp): every check is on the host, before any launch
// words up to 2^40: the partials' count stays within int and the grid within its limit
static int policy_opt_words_check(const char* fn, size_t words) {
  if (words == 0) return fail(std::string(fn) + ": words must be positive");
  if (words > ((size_t)1 << 40)) return fail(std::string(fn) + ": words must be at most 2^40");
  return 0;
}

__attribute__((visibility("default"))) int te_policy_opt_state_bytes(size_t words, size_t* out_bytes) {
  if (!out_bytes) return fail("te_policy_opt_state_bytes: null argument");
  if (policy_opt_words_check("te_policy_opt_state_bytes", words)) return 1;
  *out_bytes = opt_layout(words).bytes;
  return 0;
}

// One step's arguments: what te_policy_adam_step, te_policy_adam_step_bf16 and te_policy_ppo_epoch check and launch alike
struct AdamCall {
  float* params;
  const float* grad;
  void* state;
  size_t state_bytes, words;
  double lr, beta1, beta2, eps;
  float max_grad_norm, grad_scale;
};

static int policy_adam_check(const std::string& who, const AdamCall& c) {
  if (!c.params || !c.grad || !c.state) return fail(who + ": null argument");
  if ((uintptr_t)c.params & 15) return fail(who + ": params must be 16-byte aligned");
  if ((uintptr_t)c.grad & 15) return fail(who + ": grad must be 16-byte aligned");
  if ((uintptr_t)c.state & 15) return fail(who + ": state must be 16-byte aligned");
  if (policy_opt_words_check(who.c_str(), c.words)) return 1;
  const OptLayout o = opt_layout(c.words);
  if (c.state_bytes < o.bytes)
    return fail(who + ": state too small (" + std::to_string(c.state_bytes) + " bytes, te_policy_opt_state_bytes says " +
                std::to_string(o.bytes) + ")");
  if (!(c.lr >= 0.0) || !std::isfinite(c.lr)) return fail(who + ": lr must be finite and >= 0");
  if (!(c.beta1 >= 0.0 && c.beta1 < 1.0)) return fail(who + ": beta1 must be in [0, 1)");
  if (!(c.beta2 >= 0.0 && c.beta2 < 1.0)) return fail(who + ": beta2 must be in [0, 1)");
  if (!(c.eps > 0.0) || !std::isfinite(c.eps)) return fail(who + ": eps must be finite and > 0");
  if (!(c.max_grad_norm > 0.f)) return fail(who + ": max_grad_norm must be > 0 (INFINITY: no clipping)");
  if (!std::isfinite(c.grad_scale)) return fail(who + ": grad_scale must be finite");
  return 0;
}

// the two launches of a checked step; repack: the bf16 destinations of te_policy_adam_step_bf16, or NULL
static int policy_adam_launch(const AdamCall& c, const OptRepack* repack, void* stream) {
  const AdamArgs a{c.lr, c.beta1, c.beta2, (float)c.beta1, (float)c.beta2, (float)(1.0 - c.beta1), (float)(1.0 - c.beta2), (float)c.eps,
                   c.max_grad_norm, c.grad_scale};
  const OptView view = opt_view(c.state, c.words);
  const size_t partials = opt_layout(c.words).n_partials;
  if (stateless_launch(policy_gradnorm_kernel, partials, kOptThreads, 0, stream, view, c.grad, c.grad_scale)) return 1;
  if (repack) return stateless_launch(policy_adam_kernel<true>, partials, kOptThreads, 0, stream, view, c.params, c.grad, a, *repack);
  return stateless_launch(policy_adam_kernel<false>, partials, kOptThreads, 0, stream, view, c.params, c.grad, a, OptNoRepack{});
}

__attribute__((visibility("default"))) int te_policy_adam_step(float* params, const float* grad, void* state, size_t state_bytes, size_t words,
                                                               double lr, double beta1, double beta2, double eps, float max_grad_norm,
                                                               float grad_scale, void* stream) {
  const AdamCall c{params, grad, state, state_bytes, words, lr, beta1, beta2, eps, max_grad_norm, grad_scale};
  if (policy_adam_check("te_policy_adam_step", c)) return 1;
  return policy_adam_launch(c, nullptr, stream);
}

// The bf16 destinations of a shape's stepped words, from the pack kernels' own plans: range l is layer l's weight
static OptRepack policy_repack_plan(PolShape shape, uint16_t* weights_bf16, uint16_t* weights_bf16_t) {
  static_assert(kPolBMfmaLayers <= kOptRepackRanges, "one range per layer of the bf16 buffer");
  const PolPackPlan p = policy_pack_plan(shape);
  const PolPackTPlan t = policy_pack_t_plan(shape);
  OptRepack r{};
  for (int l = 0; l < kPolBMfmaLayers; ++l)
    r.r[l] = {p.l[l].src, p.l[l].src + t.l[l].N * p.l[l].K, p.l[l].K, p.l[l].Kp, p.l[l].dst, t.l[l].Np, pol_needs_dx(l) ? t.l[l].dst : -1};
  r.out = reinterpret_cast<__bf16*>(weights_bf16);
  r.out_t = reinterpret_cast<__bf16*>(weights_bf16_t);
  return r;
}

// te_policy_adam_step_bf16's own checks, behind policy_adam_check
static int policy_repack_check(const std::string& who, const uint16_t* weights_bf16, const uint16_t* weights_bf16_t) {
  if (!weights_bf16) return fail(who + ": weights_bf16 is required");
  if ((uintptr_t)weights_bf16 & 15) return fail(who + ": weights_bf16 must be 16-byte aligned");
  if ((uintptr_t)weights_bf16_t & 15) return fail(who + ": weights_bf16_t must be 16-byte aligned");
  return 0;
}

__attribute__((visibility("default"))) int te_policy_adam_step_bf16(float* params, const float* grad, void* state, size_t state_bytes,
                                                                    const te_policy_shape* shape, uint16_t* weights_bf16,
                                                                    uint16_t* weights_bf16_t, double lr, double beta1, double beta2, double eps,
                                                                    float max_grad_norm, float grad_scale, void* stream) {
  const int id = policy_shape_id(shape, "te_policy_adam_step_bf16");
  if (id < 0) return 1;
  const PolShape s = pol_shape(id, shape->lidar_channels);
  const AdamCall c{params, grad, state, state_bytes, (size_t)policy_layout(s).words, lr, beta1, beta2, eps, max_grad_norm, grad_scale};
  if (policy_adam_check("te_policy_adam_step_bf16", c) || policy_repack_check("te_policy_adam_step_bf16", weights_bf16, weights_bf16_t)) return 1;
  const OptRepack repack = policy_repack_plan(s, weights_bf16, weights_bf16_t);
  return policy_adam_launch(c, &repack, stream);
}

// ---- the level5 student's sphere encoder (te_sphere.hpp): every check is on the host, before any launch
static int sphere_channels_check(const std::string& who, int32_t channels) {
  if (channels != 3) return fail(who + ": channels must be 3 (the stacked observation's), not " + std::to_string(channels));
  return 0;
}

__attribute__((visibility("default"))) int te_sphere_encode_param_words(int32_t channels, size_t* out_words) {
  if (!out_words) return fail("te_sphere_encode_param_words: null argument out_words");
  if (sphere_channels_check("te_sphere_encode_param_words", channels)) return 1;
  *out_words = (size_t)sph_layout(3).words;
  return 0;
}

// the domain both sphere calls serve
static int sphere_domain_check(const std::string& who, int32_t channels, int32_t n_rows, int32_t n_spheres) {
  if (sphere_channels_check(who, channels)) return 1;
  if (n_spheres < 1 || n_spheres > kSphMaxSpheres)
    return fail(who + ": n_spheres must be in 1 .. " + std::to_string(kSphMaxSpheres) + ", not " + std::to_string(n_spheres));
  if (n_rows < 1) return fail(who + ": n_rows must be positive, not " + std::to_string(n_rows));
  if ((int64_t)n_rows * n_spheres > INT32_MAX) return fail(who + ": n_rows * n_spheres must be at most 2^31 - 1");
  return 0;
}

__attribute__((visibility("default"))) int te_sphere_encode(const float* params, int32_t channels, int32_t n_rows, int32_t n_spheres,
                                                            const float* stacked, const uint8_t* mask, float* out, void* stream) {
  const std::string who = "te_sphere_encode";
  if (sphere_domain_check(who, channels, n_rows, n_spheres)) return 1;
  if (pointers_check(who, {{"params", params, 16}, {"stacked", stacked, 16}, {"out", out, 16}})) return 1;
  // persistent workgroups: each stages the weights into LDS once and strides over the spheres
  int n_cu = 0;
  if (device_cu_count(who, &n_cu)) return 1;
  const int total = n_rows * n_spheres;
  const SphereIO io{params, stacked, mask, out, n_spheres, total};
  return stateless_launch(&sphere_encode_kernel<3>, std::min(total, n_cu), kSphThreads, sph_lds_plan(3).words * 4, stream, io);
}

// te_sphere_encode with bf16 operands (te_sphere_bf16.hpp): the packed bf16 copy of the two conv weights, and the launch
__attribute__((visibility("default"))) int te_sphere_bf16_words(int32_t channels, size_t* out_halfwords) {
  if (!out_halfwords) return fail("te_sphere_bf16_words: null argument out_halfwords");
  if (sphere_channels_check("te_sphere_bf16_words", channels)) return 1;
  *out_halfwords = (size_t)sph_bf16_layout().words;
  return 0;
}

__attribute__((visibility("default"))) int te_sphere_pack_bf16(const float* params, int32_t channels, uint16_t* out, void* stream) {
  const std::string who = "te_sphere_pack_bf16";
  if (sphere_channels_check(who, channels)) return 1;
  if (pointers_check(who, {{"params", params, 16}, {"out", out, 16}})) return 1;
  return stateless_launch(&sphere_pack_bf16_kernel, (sph_bf16_layout().words + 255) / 256, 256, 0, stream, params, reinterpret_cast<__bf16*>(out));
}

__attribute__((visibility("default"))) int te_sphere_encode_bf16(const float* params, const uint16_t* weights_bf16, int32_t channels,
                                                                 int32_t n_rows, int32_t n_spheres, const float* stacked,
                                                                 const uint8_t* mask, float* out, void* stream) {
  const std::string who = "te_sphere_encode_bf16";
  if (sphere_domain_check(who, channels, n_rows, n_spheres)) return 1;
  if (pointers_check(who, {{"params", params, 16}, {"weights_bf16", weights_bf16, 16}, {"stacked", stacked, 16}, {"out", out, 16}})) return 1;
  // persistent workgroups, two per CU at most: each holds its weight fragments in registers and strides over the spheres
  int n_cu = 0;
  if (device_cu_count(who, &n_cu)) return 1;
  const int total = n_rows * n_spheres;
  const SphereIO io{params, stacked, mask, out, n_spheres, total};
  return stateless_launch(&sphere_encode_bf16_kernel<3>, std::min<int64_t>(total, (int64_t)kSphBGroupsPerCu * n_cu), kSphThreads, 0, stream, io,
                          weights_bf16);
}

// The workspace of te_sphere_encode_grad: one partial gradient per workgroup the call can launch.  The bound on the grid does not
// depend on the device, so the size can be asked (and a short workspace refused) without one.
static size_t sphere_grad_workspace(int32_t n_rows, int32_t n_spheres) {
  const size_t groups = (size_t)std::min<int64_t>((int64_t)n_rows * n_spheres, kSphGradMaxGroups);
  return (groups * sph_layout(3).words * sizeof(float) + 255) / 256 * 256;
}

__attribute__((visibility("default"))) int te_sphere_encode_grad_workspace_bytes(int32_t channels, int32_t n_rows, int32_t n_spheres,
                                                                                 size_t* out_bytes) {
  const std::string who = "te_sphere_encode_grad_workspace_bytes";
  if (!out_bytes) return fail(who + ": null argument out_bytes");
  if (sphere_domain_check(who, channels, n_rows, n_spheres)) return 1;
  *out_bytes = sphere_grad_workspace(n_rows, n_spheres);
  return 0;
}

__attribute__((visibility("default"))) int te_sphere_encode_grad(const float* params, int32_t channels, int32_t n_rows, int32_t n_spheres,
                                                                 const float* stacked, const uint8_t* mask, const float* out,
                                                                 const float* d_out, float* grad, void* workspace, size_t workspace_bytes,
                                                                 void* stream) {
  const std::string who = "te_sphere_encode_grad";
  if (sphere_domain_check(who, channels, n_rows, n_spheres)) return 1;
  if (pointers_check(who, {{"params", params, 16}, {"stacked", stacked, 16}, {"out", out, 16}, {"d_out", d_out, 16}, {"grad", grad, 16},
                           {"workspace", workspace, 256}}))
    return 1;
  const size_t need = sphere_grad_workspace(n_rows, n_spheres);
  if (workspace_bytes < need)
    return fail(who + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, te_sphere_encode_grad_workspace_bytes says " +
                std::to_string(need) + ")");
  int n_cu = 0;
  if (device_cu_count(who, &n_cu)) return 1;
  const int total = n_rows * n_spheres, groups = std::min({total, n_cu, kSphGradMaxGroups}), words = sph_layout(3).words;
  const SphereGradIO io{params, stacked, mask, out, d_out, static_cast<float*>(workspace), n_spheres, total};
  if (stateless_launch(&sphere_encode_grad_kernel<3>, groups, kSphThreads, sph_grad_lds_plan(3).words * 4, stream, io)) return 1;
  return stateless_launch(&sphere_grad_reduce_kernel, (words + 255) / 256, 256, 0, stream, static_cast<const float*>(workspace), groups, words, grad);
}

// ---- advantage estimation (te_rollout.hpp): every check is on the host, before any launch
static bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + b_bytes && y < x + a_bytes;
}

__attribute__((visibility("default"))) int te_rollout_gae(int32_t n_steps, int32_t n_envs, const float* rewards, const float* values,
                                                          const float* dones, const float* last_value, double gamma, double gae_lambda,
                                                          float* adv, float* ret, void* stream) {
  if (!rewards || !values || !dones || !last_value || !adv || !ret) return fail("te_rollout_gae: null argument");
  if (n_steps < 1) return fail("te_rollout_gae: n_steps must be positive");
  if (n_envs < 1) return fail("te_rollout_gae: n_envs must be positive");
  if ((int64_t)n_steps * n_envs > INT32_MAX) return fail("te_rollout_gae: n_steps * n_envs must be at most 2^31 - 1");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return fail("te_rollout_gae: gamma must be in [0, 1]");
  if (!(gae_lambda >= 0.0 && gae_lambda <= 1.0)) return fail("te_rollout_gae: gae_lambda must be in [0, 1]");
  for (const void* q : {(const void*)rewards, (const void*)values, (const void*)dones, (const void*)last_value, (const void*)adv, (const void*)ret})
    if ((uintptr_t)q & 3) return fail("te_rollout_gae: float arrays must be 4-byte aligned");
  const size_t bytes = (size_t)n_steps * (size_t)n_envs * sizeof(float);
  for (const void* q : {(const void*)rewards, (const void*)values, (const void*)dones, (const void*)last_value}) {
    const size_t q_bytes = q == (const void*)last_value ? (size_t)n_envs * sizeof(float) : bytes;
    if (ranges_overlap(adv, bytes, q, q_bytes) || ranges_overlap(ret, bytes, q, q_bytes))
      return fail("te_rollout_gae: adv and ret must not alias the inputs");
  }
  if (ranges_overlap(adv, bytes, ret, bytes)) return fail("te_rollout_gae: adv and ret must not alias each other");
  const GaeArgs a{rewards, values, dones, last_value, adv, ret, n_steps, n_envs, (float)gamma, (float)(gamma * gae_lambda)};
  return stateless_launch(rollout_gae_kernel, (n_envs + kGaeThreads - 1) / kGaeThreads, kGaeThreads, 0, stream, a);
}

// n up to 2^40: the slice count stays within the grid's limit
static int adv_stats_n_check(const char* fn, int64_t n) {
  if (n < 1) return fail(std::string(fn) + ": n must be positive");
  if (n > ((int64_t)1 << 40)) return fail(std::string(fn) + ": n must be at most 2^40");
  return 0;
}

__attribute__((visibility("default"))) int te_adv_stats_workspace_bytes(int64_t n, size_t* out_bytes) {
  if (!out_bytes) return fail("te_adv_stats_workspace_bytes: null argument");
  if (adv_stats_n_check("te_adv_stats_workspace_bytes", n)) return 1;
  *out_bytes = stat_workspace_bytes(n);
  return 0;
}

static int adv_stats_check(const std::string& who, const float* x, const int64_t* index, int64_t n, const float* out_mean_std,
                           const void* workspace, size_t workspace_bytes) {
  if (!x || !out_mean_std || !workspace) return fail(who + ": null argument");
  if (adv_stats_n_check(who.c_str(), n)) return 1;
  if (((uintptr_t)x | (uintptr_t)out_mean_std) & 3) return fail(who + ": float arrays must be 4-byte aligned");
  if ((uintptr_t)index & 7) return fail(who + ": index must be 8-byte aligned");
  if ((uintptr_t)workspace & 7) return fail(who + ": workspace must be 8-byte aligned");
  const size_t need = stat_workspace_bytes(n);
  if (workspace_bytes < need)
    return fail(who + ": workspace too small (" + std::to_string(workspace_bytes) + " bytes, te_adv_stats_workspace_bytes says " +
                std::to_string(need) + ")");
  return 0;
}

// the two launches of a checked statistics call
static int adv_stats_launch(const float* x, const int64_t* index, int64_t n, float* out_mean_std, void* workspace, void* stream) {
  const size_t slices = stat_slices(n);
  double* partials = static_cast<double*>(workspace);
  if (stateless_launch(index ? adv_stats_partial_kernel<true> : adv_stats_partial_kernel<false>, slices, kStatThreads, 0, stream, x, index, n, partials))
    return 1;
  return stateless_launch(adv_stats_final_kernel, 1, kStatThreads, 0, stream, x, index, n, partials, (int64_t)slices, out_mean_std);
}

__attribute__((visibility("default"))) int te_adv_stats(const float* x, const int64_t* index, int64_t n, float* out_mean_std, void* workspace,
                                                        size_t workspace_bytes, void* stream) {
  if (adv_stats_check("te_adv_stats", x, index, n, out_mean_std, workspace, workspace_bytes)) return 1;
  return adv_stats_launch(x, index, n, out_mean_std, workspace, stream);
}

// ---- te_policy_ppo_epoch: every minibatch of an epoch, the four calls above enqueued back to back by one host loop
// The rows of minibatch k of an epoch over n_perm rows in minibatches of `batch`: perm[s .. s + b)
struct EpochSlice { int64_t s; int32_t b; };
static EpochSlice epoch_slice(int64_t n_perm, int32_t batch, int64_t k) {
  const int64_t s = k * (int64_t)batch, left = n_perm - s;
  return {s, (int32_t)(left < (int64_t)batch ? left : (int64_t)batch)};
}

// every check of te_policy_ppo_epoch, on the host: nothing is launched.  out: the calls the loop repeats
static int policy_ppo_epoch_check(const te_ppo_epoch_args* a, PolGradCall* grad_call, AdamCall* adam_call, bool* bf16) {
  const std::string who = "te_policy_ppo_epoch";
  if (!a) return fail(who + ": null argument");
  if (a->struct_size != sizeof(te_ppo_epoch_args))
    return fail(who + ": args->struct_size is " + std::to_string(a->struct_size) + ", sizeof(te_ppo_epoch_args) is " +
                std::to_string(sizeof(te_ppo_epoch_args)));
  const int id = policy_shape_id(&a->shape, who.c_str());
  if (id < 0) return 1;
  if (a->batch < 1) return fail(who + ": batch must be >= 1");
  if (a->n_perm < 1) return fail(who + ": n_perm must be >= 1");
  if (a->n_perm > ((int64_t)1 << 40)) return fail(who + ": n_perm must be at most 2^40");      // te_adv_stats's own limit; perm + s stays a pointer
  if (!a->perm) return fail(who + ": perm is required");
  if ((uintptr_t)a->perm & 7) return fail(who + ": perm must be 8-byte aligned");
  if (!a->weights_bf16 != !a->weights_bf16_t)
    return fail(who + ": weights_bf16 and weights_bf16_t go together: both NULL (the fp32 gradient and te_policy_adam_step) or both given "
                      "(te_policy_ppo_grad_bf16 and te_policy_adam_step_bf16)");
  *bf16 = a->weights_bf16 != nullptr;
  if (!a->adv_mean_std || !a->stats || !a->sums) return fail(who + ": adv_mean_std, stats and sums are required");
  if ((uintptr_t)a->sums & 3) return fail(who + ": sums must be 4-byte aligned");
  const PolShape shape = pol_shape(id, a->shape.lidar_channels);
  *grad_call = PolGradCall{*bf16, id, a->params, a->weights_bf16, a->weights_bf16_t, a->shape.lidar_channels, a->lidar, a->inertial, a->last_action,
                           {a->action, a->old_logp, a->adv, a->ret, a->adv_mean_std, a->clip_range, a->vf_coef, a->ent_coef}, a->grad, a->stats,
                           a->workspace, a->workspace_bytes};
  *adam_call = AdamCall{a->params, a->grad, a->state, a->state_bytes, (size_t)policy_layout(shape).words, a->lr, a->beta1, a->beta2, a->eps,
                        a->max_grad_norm, a->grad_scale};
  // the two sizes a minibatch has: the first one's and the last one's (the tail; the same when batch divides n_perm)
  const int64_t last = (a->n_perm - 1) / a->batch;
  for (const int64_t k : {(int64_t)0, last}) {
    const EpochSlice m = epoch_slice(a->n_perm, a->batch, k);
    if (adv_stats_check(who, a->adv, a->perm + m.s, m.b, a->adv_mean_std, a->adv_workspace, a->adv_workspace_bytes)) return 1;
    if (policy_ppo_grad_check(who, *bf16 ? "te_policy_grad_bf16_workspace_bytes" : "te_policy_grad_workspace_bytes_shaped", *grad_call, m.b,
                              a->perm + m.s))
      return 1;
  }
  if (policy_adam_check(who, *adam_call)) return 1;
  if (*bf16 && policy_repack_check(who, a->weights_bf16, a->weights_bf16_t)) return 1;
  return 0;
}

__attribute__((visibility("default"))) int te_policy_ppo_epoch(const te_ppo_epoch_args* args, void* stream) {
  PolGradCall g; AdamCall o; bool bf16;
  if (policy_ppo_epoch_check(args, &g, &o, &bf16)) return 1;
  const PolShape shape = pol_shape(g.shape_id, g.lidar_channels);
  // the tile kernel's LDS opt-in is the one step of a launch that is not a launch: taken now, so a refusal still comes before the first one
  if (bf16 ? lds_opt_in(reinterpret_cast<const void*>(kPolicyGradBf16Kernels[g.shape_id][g.lidar_channels - 2]), pol_grad_lds_plan_bf16(shape).bytes)
           : lds_opt_in(reinterpret_cast<const void*>(kPolicyGradKernels[g.shape_id][g.lidar_channels - 2]), pol_lds_plan(shape).words * 4))
    return 1;
  const OptRepack repack = policy_repack_plan(shape, args->weights_bf16, args->weights_bf16_t);
  const float* norm = opt_view(args->state, o.words).norm;
  const int64_t n_batches = (args->n_perm - 1) / args->batch + 1;
  for (int64_t k = 0; k < n_batches; ++k) {
    const EpochSlice m = epoch_slice(args->n_perm, args->batch, k);
    const int64_t* index = args->perm + m.s;
    if (adv_stats_launch(args->adv, index, m.b, args->adv_mean_std, args->adv_workspace, stream)) return 1;
    if (policy_ppo_grad_launch(g, m.b, index, stream)) return 1;
    if (policy_adam_launch(o, bf16 ? &repack : nullptr, stream)) return 1;
    if (stateless_launch(policy_epoch_sums_kernel, 1, 1, 0, stream, args->sums, args->stats, norm)) return 1;
  }
  return 0;
}

// ---- episode monitor (te_monitor.hpp): every check is on the host, before any launch
static int monitor_check(const char* who, const void* mon, size_t bytes, int32_t n_envs, int32_t n_records) {
  const std::string w(who);
  if (n_envs <= 0) return fail(w + ": n_envs must be positive");
  if (n_records < 0) return fail(w + ": n_records must be >= 0");
  if (!mon) return fail(w + ": null monitor buffer");
  if ((uintptr_t)mon & 15) return fail(w + ": the monitor buffer must be 16-byte aligned");
  const size_t need = monitor_offsets(n_envs, n_records).bytes;
  if (bytes < need)
    return fail(w + ": monitor buffer too small (" + std::to_string(bytes) + " bytes, te_monitor_bytes says " + std::to_string(need) + ")");
  return 0;
}

__attribute__((visibility("default"))) int te_monitor_layout(int32_t n_envs, int32_t n_records, te_monitor_offsets* out) {
  if (!out) return fail("te_monitor_layout: null argument");
  if (n_envs <= 0) return fail("te_monitor_layout: n_envs must be positive");
  if (n_records < 0) return fail("te_monitor_layout: n_records must be >= 0");
  *out = monitor_offsets(n_envs, n_records);
  return 0;
}

__attribute__((visibility("default"))) int te_monitor_bytes(int32_t n_envs, int32_t n_records, size_t* out_bytes) {
  if (!out_bytes) return fail("te_monitor_bytes: null argument");
  te_monitor_offsets o;
  if (n_envs <= 0) return fail("te_monitor_bytes: n_envs must be positive");
  if (n_records < 0) return fail("te_monitor_bytes: n_records must be >= 0");
  o = monitor_offsets(n_envs, n_records);
  *out_bytes = o.bytes;
  return 0;
}

__attribute__((visibility("default"))) int te_monitor_init(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, void* stream) {
  if (monitor_check("te_monitor_init", mon, bytes, n_envs, n_records)) return 1;
  TE_HIP(hipMemsetAsync(mon, 0, monitor_offsets(n_envs, n_records).bytes, (hipStream_t)stream));
  return 0;
}

__attribute__((visibility("default"))) int te_monitor_step(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, const float* reward,
                                                           const uint8_t* done, const int32_t* info, void* stream) {
  if (monitor_check("te_monitor_step", mon, bytes, n_envs, n_records)) return 1;
  if (!reward || !done || !info) return fail("te_monitor_step: null argument");
  if ((uintptr_t)reward & 3) return fail("te_monitor_step: reward must be 4-byte aligned");
  if ((uintptr_t)info & 15) return fail("te_monitor_step: info must be 16-byte aligned");
  return stateless_launch(monitor_step_kernel, (n_envs + kMonThreads - 1) / kMonThreads, kMonThreads, 0, stream, monitor_view(mon, n_envs, n_records),
                          reward, done, reinterpret_cast<const int4*>(info));
}

__attribute__((visibility("default"))) int te_monitor_stats(void* mon, size_t bytes, int32_t n_envs, int32_t n_records, te_monitor_summary* out,
                                                            int32_t reset_window, void* stream) {
  if (monitor_check("te_monitor_stats", mon, bytes, n_envs, n_records)) return 1;
  if (!out) return fail("te_monitor_stats: null argument");
  if ((uintptr_t)out & 7) return fail("te_monitor_stats: out must be 8-byte aligned");
  return stateless_launch(monitor_stats_kernel, 1, kMonThreads, 0, stream, monitor_view(mon, n_envs, n_records), out, (int)reset_window);
}

// ---- imitation dataset (te_dataset.hpp): every check is on the host, before any launch
static int dataset_geom_check(const std::string& w, const te_dataset_geom* g) {
  if (!g) return fail(w + ": null argument geom");
  if (g->channels != 3) return fail(w + ": channels must be 3, not " + std::to_string(g->channels));
  if (g->n_spheres < 1 || g->n_spheres > 8) return fail(w + ": n_spheres must be in 1 .. 8, not " + std::to_string(g->n_spheres));
  if (g->capacity < 1) return fail(w + ": capacity must be in 1 .. 2^31 - 1, not " + std::to_string(g->capacity));
  if (g->max_append_rows < 1 || g->max_append_rows > g->capacity)
    return fail(w + ": max_append_rows must be in 1 .. capacity (" + std::to_string(g->capacity) + "), not " + std::to_string(g->max_append_rows));
  return 0;
}

static int dataset_check(const std::string& w, const void* ds, size_t bytes, const te_dataset_geom* g) {
  if (dataset_geom_check(w, g)) return 1;
  if (pointers_check(w, {{"ds", ds, 16}})) return 1;
  const size_t need = dataset_offsets(*g).bytes;
  if (bytes < need) return fail(w + ": ds too small (bytes is " + std::to_string(bytes) + ", te_dataset_layout says " + std::to_string(need) + ")");
  return 0;
}

__attribute__((visibility("default"))) int te_dataset_layout(const te_dataset_geom* geom, te_dataset_offsets* out) {
  const std::string who = "te_dataset_layout";
  if (!out) return fail(who + ": null argument out");
  if (dataset_geom_check(who, geom)) return 1;
  *out = dataset_offsets(*geom);
  return 0;
}

__attribute__((visibility("default"))) int te_dataset_init(void* ds, size_t bytes, const te_dataset_geom* geom, void* stream) {
  if (dataset_check("te_dataset_init", ds, bytes, geom)) return 1;
  TE_HIP(hipMemsetAsync(ds, 0, dataset_offsets(*geom).bytes, (hipStream_t)stream));
  return 0;
}

__attribute__((visibility("default"))) int te_dataset_append(void* ds, size_t bytes, const te_dataset_geom* geom, int32_t n_rows,
                                                             const float* stacked, const uint8_t* mask, const float* inertial,
                                                             const float* last_action, const float* teacher, const uint8_t* active,
                                                             void* stream) {
  const std::string who = "te_dataset_append";
  if (dataset_check(who, ds, bytes, geom)) return 1;
  if (n_rows < 1 || n_rows > geom->max_append_rows)
    return fail(who + ": n_rows must be in 1 .. max_append_rows (" + std::to_string(geom->max_append_rows) + "), not " + std::to_string(n_rows));
  if (pointers_check(who, {{"stacked", stacked, 16}, {"mask", mask, 1}, {"inertial", inertial, 4}, {"last_action", last_action, 4},
                                   {"teacher", teacher, 4}}))
    return 1;
  const DatasetView v = dataset_view(ds, *geom);
  if (stateless_launch(dataset_scan_kernel, 1, kDsScanThreads, 0, stream, v, mask, active, (int)n_rows)) return 1;
  return stateless_launch(dataset_copy_kernel, n_rows, kDsCopyThreads, 0, stream, v, DatasetRows{stacked, mask, inertial, last_action, teacher});
}

__attribute__((visibility("default"))) int te_dataset_gather(void* ds, size_t bytes, const te_dataset_geom* geom, int32_t batch,
                                                             const int64_t* index, uint64_t seed, uint64_t draw, int32_t last_action_mode,
                                                             float noise_std, float* out_stacked, uint8_t* out_mask, float* out_inertial,
                                                             float* out_last_action, float* out_teacher, int64_t* out_index, void* stream) {
  const std::string who = "te_dataset_gather";
  if (dataset_check(who, ds, bytes, geom)) return 1;
  if (batch < 1) return fail(who + ": batch must be >= 1, not " + std::to_string(batch));
  if (last_action_mode < TE_DATASET_LA_KEEP || last_action_mode > TE_DATASET_LA_NOISE)
    return fail(who + ": last_action_mode must be 0 (keep), 1 (random) or 2 (noise), not " + std::to_string(last_action_mode));
  if (!(noise_std >= 0.f) || !std::isfinite(noise_std)) return fail(who + ": noise_std must be finite and >= 0");
  if ((uintptr_t)index & 7) return fail(who + ": index must be 8-byte aligned");
  if ((uintptr_t)out_index & 7) return fail(who + ": out_index must be 8-byte aligned");
  if (pointers_check(who, {{"out_stacked", out_stacked, 16}, {"out_mask", out_mask, 1}, {"out_inertial", out_inertial, 4},
                                   {"out_last_action", out_last_action, 4}, {"out_teacher", out_teacher, 4}}))
    return 1;
  const DatasetBatch b{out_stacked, out_mask, out_inertial, out_last_action, out_teacher, reinterpret_cast<long long*>(out_index),
                       reinterpret_cast<const long long*>(index), (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32),
                       (int)last_action_mode, noise_std};
  return stateless_launch(dataset_gather_kernel, batch, kDsCopyThreads, 0, stream, dataset_view(ds, *geom), b);
}
