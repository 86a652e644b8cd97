// Host-only check of te_policy_ppo_epoch's and te_policy_adam_step_bf16's argument validation, for a sanitizer build
// (tools/ppo_epoch_host_check.sh: te_env.hip's host code and this file under -fsanitize=address,undefined).  Every call below must be
// refused before anything is launched, so the program needs no GPU and makes no launch: it exercises the host loop's arithmetic on
// perm, n_perm and batch (the first and the tail minibatch's offsets and sizes) with NULL, short and odd inputs.  Exit status 0: every
// refusal came, with a message that starts with the entry's name.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "threatengage.h"

static int failures = 0;

static void expect_refused(int rc, const char* entry, const char* fragment, const char* what) {
  const char* err = te_last_error();
  const bool ok = rc != 0 && !strncmp(err, entry, strlen(entry)) && strstr(err, fragment);
  printf("%s %-44s %s\n", ok ? "ok  " : "FAIL", what, err);
  if (!ok) ++failures;
}

int main() {
  const char* E = "te_policy_ppo_epoch: ";
  const te_policy_shape shape{3, 256, 2, {64, 64, 0, 0}};
  size_t words = 0, state_bytes = 0, ws_bytes = 0, adv_bytes = 0;
  if (te_policy_param_words_shaped(&shape, &words) || te_policy_opt_state_bytes(words, &state_bytes) ||
      te_policy_grad_workspace_bytes_shaped(&shape, 64, &ws_bytes) || te_adv_stats_workspace_bytes(64, &adv_bytes)) {
    printf("FAIL sizes: %s\n", te_last_error());
    return 1;
  }
  // host memory stands in for the device arrays: the validation must not read it, and ASan watches the ends of perm
  std::vector<int64_t> perm(200, 0);
  alignas(256) static unsigned char blob[4096];
  void* const fake = blob;
  te_ppo_epoch_args ok{};
  ok.struct_size = sizeof(ok); ok.shape = shape; ok.params = (float*)fake;
  ok.lidar = ok.inertial = ok.last_action = ok.action = ok.old_logp = ok.adv = ok.ret = (const float*)fake;
  ok.perm = perm.data(); ok.n_perm = (int64_t)perm.size(); ok.batch = 64;
  ok.clip_range = 0.2f; ok.vf_coef = 0.5f; ok.ent_coef = 0.f;
  ok.grad = (float*)fake; ok.state = fake; ok.state_bytes = state_bytes;
  ok.lr = 3e-4; ok.beta1 = 0.9; ok.beta2 = 0.999; ok.eps = 1e-5; ok.max_grad_norm = 0.5f; ok.grad_scale = 1.f;
  ok.workspace = fake; ok.workspace_bytes = ws_bytes; ok.adv_workspace = fake; ok.adv_workspace_bytes = adv_bytes;
  ok.adv_mean_std = ok.stats = ok.sums = (float*)fake;

  expect_refused(te_policy_ppo_epoch(nullptr, nullptr), E, "null argument", "args == NULL");
  { auto a = ok; a.struct_size = 8; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "struct_size", "short struct"); }
  { auto a = ok; a.batch = 0; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "batch must be >= 1", "batch = 0"); }
  { auto a = ok; a.batch = INT32_MIN; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "batch must be >= 1", "batch = INT32_MIN"); }
  { auto a = ok; a.n_perm = 0; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "n_perm must be >= 1", "n_perm = 0"); }
  { auto a = ok; a.n_perm = INT64_MIN; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "n_perm must be >= 1", "n_perm = INT64_MIN"); }
  { auto a = ok; a.perm = nullptr; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "perm is required", "perm == NULL"); }
  { auto a = ok; a.perm = (const int64_t*)((const char*)perm.data() + 4); expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "perm must be 8-byte", "perm misaligned"); }
  { auto a = ok; a.weights_bf16 = (uint16_t*)fake; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "go together", "one bf16 buffer"); }
  { auto a = ok; a.weights_bf16_t = (uint16_t*)fake; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "go together", "the other bf16 buffer"); }
  { auto a = ok; a.sums = nullptr; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "are required", "sums == NULL"); }
  { auto a = ok; a.lidar = nullptr; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "null argument", "lidar == NULL"); }
  { auto a = ok; a.adv = nullptr; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "null argument", "adv == NULL"); }
  { auto a = ok; a.state = nullptr; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "null argument", "state == NULL"); }
  { auto a = ok; a.workspace_bytes = ws_bytes - 1; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "workspace too small", "workspace one byte short"); }
  { auto a = ok; a.adv_workspace_bytes = 0; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "workspace too small", "no statistics workspace"); }
  { auto a = ok; a.state_bytes = state_bytes - 1; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "state too small", "state one byte short"); }
  // the tail: 200 = 3 x 64 + 8; 1 row per minibatch; one minibatch larger than the permutation; the largest sizes the fields hold
  { auto a = ok; a.batch = 1; a.max_grad_norm = 0.f; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "max_grad_norm", "batch = 1, max_grad_norm = 0"); }
  { auto a = ok; a.batch = INT32_MAX; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "workspace too small", "batch = INT32_MAX: one minibatch of 200"); }
  { auto a = ok; a.batch = 199; a.clip_range = -1.f; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "workspace too small", "batch = 199: a 1-row tail, 199 rows first"); }
  { auto a = ok; a.batch = 3; a.clip_range = -1.f; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "clip_range", "batch = 3: a 2-row tail, clip_range < 0"); }
  { auto a = ok; a.batch = INT32_MAX; a.n_perm = INT64_MAX; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "at most 2^40", "batch = INT32_MAX, n_perm = INT64_MAX"); }
  { auto a = ok; a.batch = INT32_MAX; a.n_perm = (int64_t)1 << 40; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "", "batch = INT32_MAX, n_perm = 2^40"); }
  { auto a = ok; a.batch = 1; a.n_perm = (int64_t)1 << 40; a.lr = -1.0; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "lr must be", "batch = 1, n_perm = 2^40, lr < 0"); }
  { auto a = ok; a.shape.features_dim = 300; expect_refused(te_policy_ppo_epoch(&a, nullptr), E, "is not served", "unserved shape"); }

  const char* A = "te_policy_adam_step_bf16: ";
  float* const f = (float*)fake;
  uint16_t* const h = (uint16_t*)fake;
  expect_refused(te_policy_adam_step_bf16(nullptr, f, fake, state_bytes, &shape, h, h, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "null", "params == NULL");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, state_bytes, nullptr, h, h, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "null shape", "shape == NULL");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, state_bytes, &shape, nullptr, h, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "weights_bf16 is required", "weights_bf16 == NULL");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, state_bytes, &shape, h + 1, h, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "weights_bf16 must be 16-byte", "weights_bf16 misaligned");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, state_bytes, &shape, h, h + 4, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "weights_bf16_t must be 16-byte", "weights_bf16_t misaligned");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, 64, &shape, h, h, 3e-4, 0.9, 0.999, 1e-5, 0.5f, 1.f, nullptr), A, "state too small", "short state");
  expect_refused(te_policy_adam_step_bf16(f, f, fake, state_bytes, &shape, h, h, 3e-4, 0.9, 0.999, 1e-5, 0.f, 1.f, nullptr), A, "max_grad_norm", "max_grad_norm = 0");

  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
