"""Host bookkeeping of ``GST_Tacotron.Inference_Checked``: which utterances go again, the seed of each attempt, and where an attempt's
results land.  Plain Python on host values -- no device, no torch -- so that it can be driven without a GPU.

The report columns (``REPORT_FIELDS``) are those of ``gsttaco_utterance_report`` (include/gsttaco.h).
"""

REPORT_FIELDS = ("stop_step", "frames", "end_gap", "max_jump", "back_steps", "max_stall", "visited", "nonfinite")
SEED_STRIDE = 0x9E3779B97F4A7C15           # 2^64 / golden ratio: attempt k of an utterance is k strides behind its seed
MASK64 = (1 << 64) - 1


def attempt_seed(seed, k):
    """The seed of attempt ``k`` (0 = the first) of an utterance whose seed is ``seed``: (seed + k * 0x9E3779B97F4A7C15) mod 2^64."""
    return (int(seed) + int(k) * SEED_STRIDE) & MASK64


def default_accept(steps):
    """The default test of an attempt: the stop token fired (``stop_step < steps``), the attention reached the last token
    (``end_gap == 0``) and everything is finite.  None of the three is a threshold."""
    def accept(report_row, focus, i, k):
        return int(report_row[0]) < steps and int(report_row[2]) == 0 and int(report_row[7]) == 0
    return accept


def run_checked(seeds, max_attempts, run, accept):
    """Attempt 0 runs every utterance; attempt k > 0 the ones attempt k - 1 left rejected, as a smaller batch of their own, until
    none is left or ``max_attempts`` attempts are made.

    ``run(rows, seeds)`` synthesises utterances ``rows`` (ascending indices into the original batch) under ``seeds`` (one derived
    seed each), stores their outputs -- replacing what an earlier attempt stored for those rows -- and returns
    ``(report_rows, focus)`` for them, in the order of ``rows``.  ``accept(report_row, focus, i, k)`` judges utterance i's attempt k.
    Returns ``(attempts, accepted)``: per utterance the index of the attempt whose outputs are the stored ones, and whether that
    attempt was accepted (False only when ``max_attempts`` ran out)."""
    n = len(seeds)
    if max_attempts < 1:
        raise ValueError("max_attempts must be at least 1")
    attempts, accepted = [0] * n, [False] * n
    pending = list(range(n))
    for k in range(int(max_attempts)):
        if not pending:
            break
        report_rows, focus = run(list(pending), [attempt_seed(seeds[i], k) for i in pending])
        if len(report_rows) != len(pending) or len(focus) != len(pending):
            raise ValueError("run() must return one report row and one focus value per utterance it ran")
        again = []
        for j, i in enumerate(pending):
            attempts[i] = k
            accepted[i] = bool(accept(report_rows[j], focus[j], i, k))
            if not accepted[i]:
                again.append(i)
        pending = again
    return attempts, accepted
