"""The discrete decisions of te_step, held to float64 at their thresholds and ties.

Every engage form the plan can pick restates the task logic by hand (te_engage_slots.hpp, te_engage.hpp, the LDS forms of te_logic.hpp), the fast
ones on fnorm / fdist (v_sqrt_f32); every other GPU test masks the envs in which a decision sat within 1e-4 m of its threshold.  Here every form
takes ONE step without physics on the crafted states of tests/_decision_states.py and is compared, env by env, with the float64 oracle stepped on
the same blob: done, info, every integer state word, the reward (rtol 1e-5, atol 1e-3) and the float state words (1e-4).  An env that differs must
have a decision margin of at most M = 4 max(G, 2^-23 s), G from the oracle's own float32 / float64 pair (tests/test_oracle_decision_edges.py); exact
ties and integer edges may not differ at all.  A bitwise d == threshold (axis-aligned separation) is asserted on every form where the square of the
threshold is a float32 number (1, 8, 10, 20 m: the root's argument is the perfect square itself); where it is not (0.2f, 0.4f: the sum of squares
is rounded first) it is asserted on the TE_ENGAGE=lds forms (sqrtf, correctly rounded) and reported on the forms whose root is v_sqrt_f32 (1 ulp).
TE_DECISION_EDGES_RECORD=<path> appends one JSON line per case (profiles/decision_edges.json)."""
import json
import os

import numpy as np
import pytest

from tests import _decision_states as S

pytestmark = pytest.mark.gpu

# form: (shape of tests/_decision_states.py, environment knobs, the engage kernel the plan must name)
FORMS = {
    "slots": ("exp03", {}, "engage_slots_kernel<16>"),
    "regs": ("exp03", {"TE_ENGAGE": "regs"}, "engage_kernel<2, 9, false>"),
    "spw2": ("exp03", {"TE_SLOT_SPW": "2"}, "engage_slots_multi_kernel<2, true, false>"),
    "lds": ("exp03", {"TE_ENGAGE": "lds"}, "engage_observe_kernel<0, 256>"),
    "wide": ("wide", {}, "engage_kernel<6, 12, false>"),
    "wide_lds": ("wide", {"TE_ENGAGE": "lds"}, "engage_observe_kernel<0, 256>"),
    "stage02": ("stage02", {}, "engage_slots_stage02_kernel<16>"),
    "stage02_regs": ("stage02", {"TE_ENGAGE": "regs"}, "engage_stage02_kernel<2, 8>"),
    "stage02_lds": ("stage02", {"TE_ENGAGE": "lds"}, None),
    "stage01": ("stage01", {}, "engage_stage01_kernel"),
    "level5": ("level5", {}, "engage_slots_multi_kernel<2, false, false>"),
    "level5_regs": ("level5", {"TE_ENGAGE": "regs"}, "engage_kernel<6, 12, false>"),
    "level5_c1": ("level5_c1", {}, "engage_slots_multi_kernel<1, false, false>"),
    "level5_dumb": ("level5_dumb", {}, "engage_slots_multi_kernel<3, false, true>"),
    "evaluation": ("evaluation", {}, "engage_slots_kernel<16>"),
    "level5_2bt": ("level5_2bt", {}, "engage_slots_multi_kernel<2, true, false>"),
}
CASES = [(form, family) for form in FORMS for family in S.families(FORMS[form][0])]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return torch


def _env(monkeypatch, cfg, knobs, kernel):
    from dronechase_amd._lib import kernel_plan
    from dronechase_amd.batched_env import BatchedEnv
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    plan = kernel_plan(cfg)
    assert plan["engage"] == kernel or (kernel is None and "engage_observe_kernel" in plan["engage"]), plan
    env = BatchedEnv(cfg, "cuda:0")
    for k in knobs:
        monkeypatch.delenv(k)
    return env


@pytest.mark.parametrize("form,family", CASES)
def test_step_decisions_against_float64(monkeypatch, form, family):
    torch = _torch()
    shape, knobs, kernel = FORMS[form]
    r = S.reference(shape, family)
    c = r["case"]
    N = c["N"]
    env = _env(monkeypatch, c["cfg"], knobs, kernel)
    assert env.state_words() == c["blob"].size
    env.set_state(torch.from_numpy(c["blob"].view(np.int32)).cuda())
    if c["cfg"].agent_scripted and c["cfg"].stacked_obs:
        out = env.step_students()
    elif c["cfg"].stacked_obs:
        out = env.step_stacked(torch.zeros((N, 4), dtype=torch.float32, device="cuda:0"), terminal=False)
    else:
        out = env.step(torch.zeros((N, 4), dtype=torch.float32, device="cuda:0"), terminal=False)
    reward, done, info = (x.cpu().numpy() for x in out[-3:])
    got = dict(reward=reward, done=done, info=info, state=S.state_part(c, env.get_state().cpu().numpy().view(np.uint32)))
    env.close()
    bad = S.differs(c, got, r["f64"])
    on_sqrtf = knobs.get("TE_ENGAGE") == "lds"
    fig = S.figures(c, bad, None if on_sqrtf else c["rim_rounded"])
    rim = (f"{int(c['rim_exact'].sum())} envs, all asserted" if on_sqrtf else
           f"{int(c['rim_exact'].sum())} envs, {int(c['rim_rounded'].sum())} of them on a rounded square and reported: {fig['rim_exact_disagreeing']} disagree")
    print(f"{form}/{family}: M = {fig['M']:.3g} m, held = {fig['held_share']:.3f}, the kernel disagrees in {fig['disagreeing']} envs up to "
          f"{fig['largest_disagreeing_margin']:.3g} m, agrees down to {fig['smallest_agreeing_margin']}; bitwise d == threshold: {rim}")
    path = os.environ.get("TE_DECISION_EDGES_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(fig, form=form, engage=kernel, pair_G_case=r["G"])) + "\n")
    why = [(e, str(c["tag"][e]), float(c["margin"][e])) for e in fig["unexcused"][:8]]
    assert not fig["unexcused"], f"{form}/{family}: the kernel decides differently from float64 where nothing excuses it (env, case, margin): {why}"
    assert fig["held_share"] >= 0.6
