"""A Monte Carlo sweep on one Batch: generate -> run -> stats -> clear over blocks of
seeds, the statistics reduced on the device (Batch.stats, hge_batch_stats) so that nothing
per event crosses to the host.  Pure host code around engine.Batch's calls."""
import numpy as np

from .engine import STATS_ROW_DTYPE, Batch, StatsSpec


def sweep(n, events, k, graphs, batches, seed, forkers=0, fork_p=0.0, cascade_p=0.0, op_lag=0, spec=None, device=0):
    """`batches` batches of `graphs` generated graphs each (batch i: the seeds
    seed + i * graphs ..., gossip.counter_gossip's streams under gossip.schedule(., k)) on
    one Batch of n participants, whose allocations the batches share.  Returns
    dict(graphs= the per-graph rows of every batch concatenated in seed order (the
    structured array of Batch.stats), round=, call=, lag=, ts=, hist= the histograms summed
    over all of them, ordered= the events ordered in all, fallbacks= the graphs replayed
    call by call, spec= the StatsSpec used)."""
    b = Batch(n, device)
    try:
        spec = StatsSpec(lag_bin=n) if spec is None else spec
        rows, hist, ordered, fallbacks = [], None, 0, 0
        for i in range(batches):
            b.generate(events, k, graphs, seed + i * graphs, forkers, fork_p, cascade_p, op_lag)
            ordered += b.run()
            fallbacks += b.fallbacks()
            st = b.stats(spec)
            rows.append(st["graphs"])
            hist = st["hist"] if hist is None else hist + st["hist"]
            b.clear()
    finally:
        b.close()
    if hist is None:
        hist = np.zeros(spec.hist_len(), np.int64)
    out = dict(graphs=np.concatenate(rows) if rows else np.zeros(0, STATS_ROW_DTYPE), hist=hist, ordered=ordered,
               fallbacks=fallbacks, spec=spec)
    out.update(spec.split(hist))
    return out


def quantile(hist, q, lo, width):
    """The bin that holds the q-quantile of a histogram whose bin i covers
    [lo + i * width, lo + (i + 1) * width): its edges (left, right), the smallest bin at
    which the cumulative count reaches q of the total (q in [0, 1]; q = 0: the first
    non-empty bin).  A clamped last bin has no right edge of its own: read (left, right)
    there as `left or more`.  For the ts histogram pass hist[1:-1] (bin 0 lies below ts_lo)
    or account for the shift by one.  None for an empty histogram."""
    h = np.asarray(hist, np.int64)
    total = int(h.sum())
    if total == 0:
        return None
    need = max(1, int(np.ceil(q * total)))
    i = int(np.searchsorted(np.cumsum(h), need, side="left"))
    return lo + i * width, lo + (i + 1) * width
