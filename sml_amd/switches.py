"""Every SML_* environment variable the Python package reads: name -> (default, meaning).  get(name) is the one accessor;
an undeclared name raises KeyError.  Values are the environment's strings (None: unset); callers convert them, and each
reads at the moment it always did -- class attributes at import, the rest per call or per engine.
(The library's own switches: struct Switches in csrc/capi.hip.  INTEGRATION.md's table lists both.)"""
import os

SWITCHES = {
    "SML_COMM": ("peer", "carrier of the multi-GPU exchanges: peer | rccl | torch"),
    "SML_PEER_TIMEOUT_S": ("120", "hang guard of the peer polls, seconds"),
    "SML_PEER_CHECK_ROUNDS": ("6", "rounds of the peer exchange's start-up self-check"),
    "SML_DEBUG_PEER": (None, "set: report the step at which the peer exchange's set-up failed"),
    "SML_FLAG_TIMEOUT_S": ("300", "hang guard of the evaluation hand-off flag, seconds"),
    "SML_EVAL": ("blocked", "rank kernel of large test sets: blocked | sliced | plain"),
    "SML_EVAL_TRANSFERRED": ("1", "0: evaluation-only updata() forwards run on the training stream"),
    "SML_TRANSFERRED_MAX_BYTES": (str(24 << 30), "budget of the ring of transferred tables kept for evaluation"),
    "SML_SIDE_EVAL_CUS": ("-1", "CUs of the evaluation partition (-1: a quarter of the chip; 0: a low-priority stream)"),
    "SML_SIDE_EVAL_WGS": ("0", "grid cap of a side-stream evaluation (0: none)"),
    "SML_TRAIN_PARTITION": ("1", "0: training on all CUs"),
    "SML_SIDE_SYNC": ("flag", "event: cross-queue events instead of flag kernels"),
    "SML_PREP_CUS": ("0", "k > 0: the bare step's index preparation confined to the last k CUs"),
    "SML_PREP_PRIO": ("", "low | high: priority of the index-preparation stream"),
    "SML_TR_SPECULATE": ("1", "0: the driver samples every transfer-stage pass in place"),
    "SML_FORCE_DIST": (None, "1: a one-rank process group takes the distributed code paths (tests)"),
    "SML_ONE_DEVICE": (None, "1: all ranks on device 0 (tests)"),
    "SML_LAUNCHED": (None, "1: this process is a rank (set by the launcher for its children)"),
    "SML_JOB_TIMEOUT_S": (None, "seconds before the launcher stops the rank processes and exits 124"),
    "SML_FAULT_DUMP_S": (None, "seconds after which the CLI dumps all threads' Python stacks once"),
    "SML_HOST_THREADS": ("1", "torch host threads of the CLI process"),
    "SML_EXTRA_FLAGS": ("", "extra hipcc flags of a measurement build"),
}


def get(name):
    return os.environ.get(name, SWITCHES[name][0])
