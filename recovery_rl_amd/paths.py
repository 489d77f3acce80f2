"""Which code a run takes: the boolean RRL_* switches (one table, one reader) and the decisions made from them -- the update
path, the acting pass of the SQRL and Q-sampling lines, the evaluation rollout, what seed packing refuses.  Pure Python: no
torch, no library.  A new line or scoring mode is a row of SWITCHES, a list of requirements and a row of fast_update.ACT_ENTRIES.
"""
import os
from collections import namedtuple

Switch = namedtuple("Switch", "name rule read doc")

# the three parsing rules (of the variable's value, "" when unset)
ON, NOT_OFF, SET = '== "1"', '!= "0"', 'not in ("", "0")'
_RULES = {ON: lambda v: v == "1", NOT_OFF: lambda v: v != "0", SET: lambda v: v not in ("", "0")}
# when a switch is read
IMPORT, LOOP, EXPERIMENT, CALL = "import", "loop build", "Experiment build", "each call"

SWITCHES = (
    Switch("RRL_FAST_BASELINES", ON, CALL, "The comparison algorithms (LR, RSPO, SQRL, RCPO) take the fused update path too."),
    Switch("RRL_FAST_SQRL", ON, LOOP, "SQRL's constraint-sampling acting pass runs on the rrl_sqrl_act kernel (sqrl_acting_path)."),
    Switch("RRL_PACK_SQRL", ON, CALL, "--seeds_per_gpu packs SQRL, its acting pass as one rrl_sqrl_act_packed launch (read in "
           "experiment.run_packed; needs sqrl_acting_path(cfg) == \"hip\" and at most 8 seeds)."),
    Switch("RRL_SQRL_F16X3", ON, LOOP, "The rrl_sqrl_act pass scores its candidates with layer 2 of Q_risk in f16x3 "
           "(rrl_sqrl_act_f16x3); it matters only where sqrl_acting_path(cfg) == \"hip\"."),
    Switch("RRL_FAST_QSAMPLE", ON, LOOP, "The acting pass of --Q_sampling_recovery runs on the rrl_qsample_act kernels "
           "(qsample_acting_path)."),
    Switch("RRL_PACK_QSAMPLE", ON, LOOP, "That pass evaluates the recovery gate inside the qsample call (rrl_qsample_act_gated: "
           "three launches the tape records), and --seeds_per_gpu packs the line as one rrl_qsample_act_packed stage (read again in "
           "experiment.run_packed; needs qsample_acting_path(cfg) == \"hip\" and at most 8 seeds)."),
    Switch("RRL_QSAMPLE_F16X3", ON, LOOP, "The rrl_qsample_act pass scores its candidates with layer 2 of Q_risk in f16x3 "
           "(rrl_qsample_act_f16x3); only where qsample_acting_path(cfg) == \"hip\", and the random-action phase keeps its f32 code."),
    Switch("RRL_FAST_EVAL", ON, CALL, "Policy evaluation is one rrl_eval_rollout launch (eval_rollout_path, read at every evaluation)."),
    Switch("RRL_FAST_EVAL_MAZE", ON, CALL, "On top of RRL_FAST_EVAL=1: Maze evaluates on rrl_eval_rollout_maze."),
    Switch("RRL_FAST_EVAL_QSAMPLE", ON, CALL, "On top of RRL_FAST_EVAL=1: --Q_sampling_recovery evaluates on rrl_eval_rollout_qs, "
           "whatever RRL_FAST_QSAMPLE says."),
    Switch("RRL_FAST_EVAL_SQRL", ON, CALL, "On top of RRL_FAST_EVAL=1: --use_constraint_sampling evaluates on rrl_eval_rollout_sqrl, "
           "whatever RRL_FAST_SQRL says."),
    Switch("RRL_EVAL_SQRL_F16X3", ON, EXPERIMENT, "The SQRL evaluation scores its candidates in f16x3 (rrl_eval_rollout_sqrl_f16x3), "
           "independent of RRL_SQRL_F16X3; kept as Experiment.eval_f16x3_switches and used from then on."),
    Switch("RRL_EVAL_QSAMPLE_F16X3", ON, EXPERIMENT, "The Q-sampling evaluation scores its candidates in f16x3 "
           "(rrl_eval_rollout_qs_f16x3), independent of RRL_QSAMPLE_F16X3; kept as Experiment.eval_f16x3_switches likewise."),
    Switch("RRL_W2_FRAG", NOT_OFF, EXPERIMENT + " (FlatNet) and " + CALL + " (the path functions)", "The 256-wide nets keep W2 a "
           "second time in MFMA fragment order, which the acting kernels need; 0: A/B runs of profiles/."),
    Switch("RRL_CARRY_ACTOR", NOT_OFF, LOOP, "Two of the acting pass's forwards ride in the Q_risk update's launches; 0: the pass's "
           "own two launches (A/B and the bit-identity test)."),
    Switch("RRL_DRAW_AHEAD", NOT_OFF, LOOP, "The task batch's keys are selected one step ahead, without a draw launch "
           "(FastUpdater.update_pair); 0: off."),
    Switch("RRL_PLAN_F16X3", SET, CALL, "A FusedPlanner built without an explicit f16x3 evaluates the hidden layers as three f16 "
           "MFMA products of hi / lo splits."),
    Switch("RRL_ROCTX", SET, IMPORT, "roctx ranges around the stages of the lock-step iteration (utils.trace_range), for marker "
           "traces of the eager loop."),
    Switch("RRL_DIST_FORCE_INIT", SET, CALL, "distributed.init() makes a 1-rank process group, so that every collective really goes "
           "through the backend."),
)
_ROW = {s.name: s for s in SWITCHES}


def switch(name):
    """The value of the switch `name` in the environment now, by its row's rule."""
    return _RULES[_ROW[name].rule](os.environ.get(name, ""))


def _named(name):
    return lambda: switch(name)


# the ON switches by the names the tests and profiles/ know them under
fast_baselines_enabled = _named("RRL_FAST_BASELINES")
fast_sqrl_enabled, pack_sqrl_enabled, sqrl_f16x3_enabled = map(_named, ("RRL_FAST_SQRL", "RRL_PACK_SQRL", "RRL_SQRL_F16X3"))
fast_qsample_enabled, pack_qsample_enabled, qsample_f16x3_enabled = map(
    _named, ("RRL_FAST_QSAMPLE", "RRL_PACK_QSAMPLE", "RRL_QSAMPLE_F16X3"))
fast_eval_enabled, fast_eval_maze_enabled, fast_eval_qsample_enabled, fast_eval_sqrl_enabled = map(
    _named, ("RRL_FAST_EVAL", "RRL_FAST_EVAL_MAZE", "RRL_FAST_EVAL_QSAMPLE", "RRL_FAST_EVAL_SQRL"))
eval_sqrl_f16x3_enabled, eval_qsample_f16x3_enabled = map(_named, ("RRL_EVAL_SQRL_F16X3", "RRL_EVAL_QSAMPLE_F16X3"))


# -- the update path -----------------------------------------------------------------------------------------------------
BASELINE_FLAGS = ("DGD_constraints", "update_nu", "nu_schedule", "use_constraint_sampling", "RCPO")


def uses_baseline_terms(cfg):
    return any(bool(getattr(cfg, f, False)) for f in BASELINE_FLAGS)


def fast_path_supported(cfg):
    """The fused path covers the Recovery-RL configurations (task SAC + Q_risk, model-free or
    model-based recovery, reward penalty); the comparison algorithms (BASELINE_FLAGS) use the autograd path
    unless RRL_FAST_BASELINES=1."""
    return (cfg.policy == "Gaussian" and not cfg.automatic_entropy_tuning
            and (switch("RRL_FAST_BASELINES") or not uses_baseline_terms(cfg))
            and cfg.target_update_interval == 1 and not getattr(cfg, "cnn", False))


def fused_256(cfg):
    """The fused update path, taken (no --no_fast_path), at the hidden width the acting and evaluation kernels are built for."""
    return fast_path_supported(cfg) and not getattr(cfg, "no_fast_path", False) and int(cfg.hidden_size) == 256


# -- the two candidate-scoring lines ------------------------------------------------------------------------------------------
def sqrl_line(cfg):
    """SAC._sqrl_action on every step: --use_constraint_sampling without a recovery policy."""
    return bool(cfg.use_constraint_sampling) and not cfg.use_recovery


def qsample_line(cfg):
    """Q-sampling candidates for the gated steps: --use_recovery --Q_sampling_recovery without --MF_recovery (model-free wins in
    the module code) and without --use_constraint_sampling."""
    return (bool(cfg.use_recovery) and bool(getattr(cfg, "Q_sampling_recovery", False)) and not cfg.MF_recovery
            and not cfg.use_constraint_sampling)


eval_sqrl_line, eval_qsample_line = sqrl_line, qsample_line

# What a line's acting pass needs to run on its kernels, in the order seed packing names what is missing: (holds(cfg, S), the
# refusal's text).  The pass is "hip" when all hold for one seed; the last entry is the limit of the packed form.
FRAG_MAX_SEEDS = 8          # packed runs keep the nets' fragment-order W2 copies up to this many seeds (packed.PackedLoop)
_REST = " (Gaussian policy, fixed alpha, --target_update_interval 1, no --no_fast_path, RRL_W2_FRAG not 0)"
_SEEDS = (lambda cfg, S: S <= FRAG_MAX_SEEDS,
          "at most %(max)d seeds per GPU (its launch reads Q_risk's fragment-order W2 copy, which packed runs keep up to that many "
          "seeds; got %(S)d)")
SQRL_NEEDS = (
    (lambda cfg, S: switch("RRL_FAST_SQRL"), "the acting pass on the rrl_sqrl_act kernel: set RRL_FAST_SQRL=1"),
    (lambda cfg, S: switch("RRL_FAST_BASELINES"), "the fused update path: set RRL_FAST_BASELINES=1"),
    (lambda cfg, S: not cfg.use_recovery,
     "a run without a recovery policy (--use_recovery takes SQRL's acting pass through module code)"),
    (lambda cfg, S: int(cfg.hidden_size) == 256, "--hidden_size 256 (the kernel's Q_risk width; got %(hidden)d)"),
    (lambda cfg, S: sqrl_line(cfg) and fused_256(cfg) and switch("RRL_W2_FRAG"), "the acting pass on the rrl_sqrl_act kernel" + _REST),
    _SEEDS)
QSAMPLE_NEEDS = (
    (lambda cfg, S: switch("RRL_FAST_QSAMPLE"), "the acting pass on the rrl_qsample_act kernels: set RRL_FAST_QSAMPLE=1"),
    (lambda cfg, S: not cfg.MF_recovery,
     "a run without --MF_recovery (the model-free recovery policy wins over --Q_sampling_recovery, and packs without this switch)"),
    (lambda cfg, S: not cfg.use_constraint_sampling, "a run without --use_constraint_sampling (SQRL's acting pass is another one)"),
    (lambda cfg, S: int(cfg.hidden_size) == 256, "--hidden_size 256 (the kernels' Q_risk width; got %(hidden)d)"),
    (lambda cfg, S: qsample_line(cfg) and fused_256(cfg) and switch("RRL_W2_FRAG"),
     "the acting pass on the rrl_qsample_act kernels" + _REST),
    _SEEDS)
# PackedLoop's own refusal of a tenth seed, by the loop flag that marks the line
PACKED_SEED_LIMITS = tuple(
    (flag, what + " packs at most %d seeds per GPU: it reads the fragment-order W2 copy of Q_risk, which packed runs keep up to "
     "that many seeds only (got %d)")
    for flag, what in (("sqrl_hip", "SQRL's constraint-sampling acting pass (rrl_sqrl_act_packed)"),
                       ("qsample_hip", "the Q-sampling recovery acting pass (rrl_qsample_act_packed)")))


def missing(needs, cfg, S=1):
    """The text of the first of `needs` that does not hold for S seeds of cfg, or None."""
    for holds, text in needs:
        if not holds(cfg, S):
            return text % {"hidden": int(cfg.hidden_size), "max": FRAG_MAX_SEEDS, "S": S}
    return None


def sqrl_acting_path(cfg):
    """Where the training actions of --use_constraint_sampling come from: "hip" (FastActor.act_sqrl) under RRL_FAST_SQRL=1
    on the fused path (RRL_FAST_BASELINES=1), without a recovery policy, at hidden width 256; else "modules"
    (SAC._sqrl_action), which evaluation, the one-state call and every other configuration keep."""
    return "modules" if missing(SQRL_NEEDS, cfg) else "hip"


def qsample_acting_path(cfg):
    """Where the recovery actions of --use_recovery --Q_sampling_recovery come from in the training loop: "hip"
    (FastActor.act_qsample) under RRL_FAST_QSAMPLE=1 on the fused path at hidden width 256; else "modules"
    (QRiskWrapper.select_action), which evaluation, the one-state call and every other configuration keep."""
    return "modules" if missing(QSAMPLE_NEEDS, cfg) else "hip"


def sqrl_scoring(cfg):
    """The arithmetic of the kernel acting pass's scores: "f16x3" under RRL_SQRL_F16X3=1 where sqrl_acting_path(cfg) == "hip",
    else "f32" (the module path's too)."""
    return "f16x3" if switch("RRL_SQRL_F16X3") and sqrl_acting_path(cfg) == "hip" else "f32"


def qsample_scoring(cfg):
    """The same for the Q-sampling line, under RRL_QSAMPLE_F16X3=1 (evaluation has a switch of its own: eval_scoring)."""
    return "f16x3" if switch("RRL_QSAMPLE_F16X3") and qsample_acting_path(cfg) == "hip" else "f32"


# -- what a lock-step loop runs (read once, when it is built) ---------------------------------------------------------------
Acting = namedtuple("Acting", "sqrl_hip sqrl_f16x3 qsample_hip qsample_gated qsample_f16x3")
ACTING_RULES = ("sqrl_acting", "sqrl_scoring", "qsample_acting", "qsample_scoring", "qsample_gate")


def acting(cfg, have_fast, have_w2p):
    """The acting pass of a loop on cfg whose agent has (or has not) the fused path and Q_risk's fragment-order W2 copy: each
    line on its kernels or not, then -- only where it is -- its f16x3 scores and, for Q-sampling, the gate inside the call."""
    sqrl = bool(have_fast and sqrl_acting_path(cfg) == "hip" and have_w2p)
    qsample = bool(have_fast and qsample_acting_path(cfg) == "hip" and have_w2p)
    return Acting(sqrl, sqrl and switch("RRL_SQRL_F16X3"), qsample, qsample and switch("RRL_PACK_QSAMPLE"),
                  qsample and switch("RRL_QSAMPLE_F16X3"))


def acting_rules(cfg, a):
    """The vector_rules entries (keys: ACTING_RULES) that say what `a` -- an Acting, or the loop that stores its fields -- runs:
    which code draws, scores and picks a line's candidates in the training loop, the arithmetic of the scores, and where the
    Q-sampling pass evaluates its recovery gate."""
    rules = {}
    if cfg.use_constraint_sampling:
        rules.update(sqrl_acting="hip" if a.sqrl_hip else "modules", sqrl_scoring="f16x3" if a.sqrl_f16x3 else "f32")
    if cfg.use_recovery and cfg.Q_sampling_recovery and not cfg.MF_recovery:
        rules.update(qsample_acting="hip" if a.qsample_hip else "modules", qsample_scoring="f16x3" if a.qsample_f16x3 else "f32")
        if a.qsample_gated:
            rules["qsample_gate"] = "in_launch"
    return rules


# -- evaluation ---------------------------------------------------------------------------------------------------------------
def eval_rollout_path(cfg):
    """Where Experiment.get_test_rollout_vectorized runs: "hip" (EvalRollout: one launch) under RRL_FAST_EVAL=1 on the fused
    path at hidden width 256, Navigation 1 / 2 -- or Maze with RRL_FAST_EVAL_MAZE=1 as well --, the lock-step loop, without
    a recovery policy, with the model-free one, -- with RRL_FAST_EVAL_QSAMPLE=1 as well -- with Q-sampling recovery, or -- with
    RRL_FAST_EVAL_SQRL=1 as well -- SQRL without a recovery policy; else "modules" (the loop's act() on the torch modules and
    the eager env), which SQRL with a recovery policy, model-based recovery and every other configuration keep."""
    envs = ("navigation1", "navigation2") + (("maze",) if switch("RRL_FAST_EVAL_MAZE") else ())
    common = (switch("RRL_FAST_EVAL") and fused_256(cfg) and cfg.env_name in envs and int(getattr(cfg, "num_envs", 1)) > 1)
    if cfg.use_constraint_sampling:
        hip = common and switch("RRL_FAST_EVAL_SQRL") and sqrl_line(cfg)
    else:
        hip = common and (not cfg.use_recovery or bool(cfg.MF_recovery) or (switch("RRL_FAST_EVAL_QSAMPLE") and qsample_line(cfg)))
    return "hip" if hip else "modules"


def eval_f16x3_switches():
    """(RRL_EVAL_SQRL_F16X3, RRL_EVAL_QSAMPLE_F16X3) now."""
    return switch("RRL_EVAL_SQRL_F16X3"), switch("RRL_EVAL_QSAMPLE_F16X3")


def eval_scoring(cfg, switches=None):
    """The arithmetic of the evaluation rollout's candidate scores: "f16x3" on the SQRL line under RRL_EVAL_SQRL_F16X3=1 and on
    the Q-sampling line under RRL_EVAL_QSAMPLE_F16X3=1, where eval_rollout_path(cfg) == "hip"; else "f32" (the module path's
    too, and every configuration that scores no candidates).  `switches` = (SQRL, Q-sampling): the two switches as read
    earlier (an Experiment's, from when its loop was built); None: the environment now."""
    sqrl, qsample = eval_f16x3_switches() if switches is None else switches
    if eval_rollout_path(cfg) != "hip":
        return "f32"
    return "f16x3" if (sqrl_line(cfg) and sqrl) or (qsample_line(cfg) and qsample) else "f32"      # (the lines exclude each other)
