// te_policy_host.hpp — the host path the policy kernels share (included by te_env.hip ahead of its extern "C" region): the launch geometry,
// the tables of served kernel instances, the shape lookup, the bf16 packing and the loss inputs.  The tables stay ahead of te_create and
// the entries (te_abi_stateless.hpp) behind the env's: a kernel instance's place in the code object follows its first use here.
#pragma once
#include "te_host.hpp"

// The geometry of a policy kernel's launch, read from the LDS plan that applies (pol_lds_plan for the fp32 tables, with kPolThreads;
// pol_lds_plan_bf16 / pol_grad_lds_plan_bf16 for the bf16 ones): M rows per workgroup, so ceil(rows / M) workgroups.
struct PolGeom {
  int M, threads, lds_bytes;
  int groups(int rows) const { return (rows + M - 1) / M; }
};
static PolGeom pol_geom(const PolLds& l) { return {l.M, kPolThreads, l.words * 4}; }
template <class LdsB>
static PolGeom pol_geom(const LdsB& l) { return {l.M, l.threads, l.bytes}; }

// a caller's buffers bound to their layouts
static PolicyParams policy_params(PolShape s, const float* params) { PolicyParams P = policy_layout(s); P.base = params; return P; }
static PolicyBf16 policy_weights(PolShape s, const uint16_t* weights) { PolicyBf16 W = policy_bf16_layout(s); W.base = weights; return W; }
static PolicyBf16 policy_weights_t(PolShape s, const uint16_t* weights_t) { PolicyBf16 W = policy_bf16_t_layout(s); W.base = weights_t; return W; }

// every served instance of a policy kernel template K<C, shape id>: table[shape id][C - 2]
template <class... Args>
using PolKernel = void (*)(PolicyParams, Args...);
#define TE_POL_INSTANCES(K) \
  {{&K<2, POL_SHAPE_DEFAULT>, &K<3, POL_SHAPE_DEFAULT>}, {&K<2, POL_SHAPE_BO>, &K<3, POL_SHAPE_BO>}, {&K<2, POL_SHAPE_LEARN>, &K<3, POL_SHAPE_LEARN>}}
static_assert(POL_SHAPE_COUNT == 3, "TE_POL_INSTANCES lists every shape");
static const PolKernel<PolicyIO> kPolicyActKernels[POL_SHAPE_COUNT][2] = TE_POL_INSTANCES(policy_act_kernel);
static const PolKernel<PolicyIn, Params, int, float*> kPolicyDriveKernels[POL_SHAPE_COUNT][2] = TE_POL_INSTANCES(policy_drive_kernel);
static const PolKernel<PolicyIn, GradTileArgs> kPolicyGradKernels[POL_SHAPE_COUNT][2] = TE_POL_INSTANCES(policy_grad_tile_kernel);
// te_policy_act_bf16's instances (te_policy_bf16.hpp) and te_policy_ppo_grad_bf16's tile kernel (te_policy_grad_bf16.hpp)
static const PolKernel<PolicyBf16, PolicyIO> kPolicyActBf16Kernels[POL_SHAPE_COUNT][2] = TE_POL_INSTANCES(policy_act_bf16_kernel);
static const PolKernel<PolicyBf16, PolicyBf16, PolicyIn, GradTileArgsB> kPolicyGradBf16Kernels[POL_SHAPE_COUNT][2] =
    TE_POL_INSTANCES(policy_grad_bf16_tile_kernel);
// te_drive_wingman_bf16's instances (te_wingman.hpp)
static const PolKernel<PolicyBf16, PolicyIn, Params, int, float*> kPolicyDriveBf16Kernels[POL_SHAPE_COUNT][2] = TE_POL_INSTANCES(policy_drive_bf16_kernel);

static std::string shape_text(const PolShape& s) {
  std::string t = "features_dim " + std::to_string(s.F) + ", hidden";
  for (int i = 0; i < s.n_hidden; ++i) t += (i ? ", " : " ") + std::to_string(s.h[i]);
  return t;
}

// The id of a served shape, or -1 with the message in g_err.  Host only: no device call.
static int policy_shape_id(const te_policy_shape* s, const char* fn) {
  const std::string who = std::string(fn) + ": ";
  if (!s) return fail(who + "null shape"), -1;
  std::string served = "; the served shapes, for lidar_channels 2 and 3:";
  for (int id = 0; id < POL_SHAPE_COUNT; ++id) served += (id ? " | " : " ") + shape_text(pol_shape(id, 3));
  if (s->lidar_channels != 2 && s->lidar_channels != 3)
    return fail(who + "lidar_channels must be 2 or 3, not " + std::to_string(s->lidar_channels) + served), -1;
  if (s->n_hidden < 1 || s->n_hidden > 3) return fail(who + "n_hidden must be 1, 2 or 3, not " + std::to_string(s->n_hidden) + served), -1;
  bool f_known = false;
  for (int id = 0; id < POL_SHAPE_COUNT; ++id) {
    const PolShape t = pol_shape(id, s->lidar_channels);
    if (t.F != s->features_dim) continue;
    f_known = true;
    bool same = t.n_hidden == s->n_hidden;
    for (int i = 0; same && i < t.n_hidden; ++i) same = t.h[i] == s->hidden[i];
    if (same) return id;
  }
  if (!f_known) return fail(who + "features_dim " + std::to_string(s->features_dim) + " is not served" + served), -1;
  std::string h;
  for (int i = 0; i < s->n_hidden; ++i) h += (i ? ", " : "") + std::to_string(s->hidden[i]);
  return fail(who + "hidden [" + h + "] is not served with features_dim " + std::to_string(s->features_dim) + served), -1;
}

// The element count of one of a served shape's buffers (layout: policy_layout, policy_bf16_layout or policy_bf16_t_layout)
template <class Layout>
static int policy_shaped_words(const char* fn, const te_policy_shape* shape, size_t* out, Layout layout) {
  if (!out) return fail(std::string(fn) + ": null argument");
  const int id = policy_shape_id(shape, fn);
  if (id < 0) return 1;
  *out = (size_t)layout(pol_shape(id, shape->lidar_channels)).words;
  return 0;
}

// The bf16 copy of a served shape's weights: one thread per element of the plan (plan_of: policy_pack_plan or policy_pack_t_plan, with its kernel)
template <class Plan, class Kernel>
static int policy_pack(const char* fn, const float* params, const te_policy_shape* shape, uint16_t* out, void* stream, Plan (*plan_of)(PolShape),
                       Kernel kernel) {
  const std::string who = std::string(fn);
  const int id = policy_shape_id(shape, fn);
  if (id < 0) return 1;
  if (!params || !out) return fail(who + ": null argument");
  if ((uintptr_t)params & 15) return fail(who + ": params must be 16-byte aligned");
  if ((uintptr_t)out & 15) return fail(who + ": out must be 16-byte aligned");
  const Plan plan = plan_of(pol_shape(id, shape->lidar_channels));
  return stateless_launch(kernel, (plan.total + 255) / 256, 256, 0, stream, params, plan, reinterpret_cast<__bf16*>(out));
}

// The per-row inputs and the coefficients of PPO's loss, as the gradient entries get them, and their place in the tile kernel's arguments
struct PolLossInputs {
  const float *action, *old_logp, *adv, *ret, *adv_mean_std;
  float clip_range, vf_coef, ent_coef;
};

template <class TileArgs>   // GradTileArgs or GradTileArgsB
static void policy_loss_inputs(TileArgs& t, const PolLossInputs& in, int32_t n) {
  t.action = in.action; t.old_logp = in.old_logp; t.adv = in.adv; t.ret = in.ret; t.adv_mean_std = in.adv_mean_std;
  t.clip = in.clip_range; t.vf_coef = in.vf_coef; t.ent_coef = in.ent_coef; t.inv_n = 1.f / (float)n;
}
