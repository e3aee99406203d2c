"""numpy restatement of `tw_joint_histogram` / `evaluate.joint_histograms`: the counts are np.histogramdd on float64 casts, the
three outside counters direct numpy predicates.  Shared by tests/test_joint_histogram_cpu.py and tests/test_joint_histogram_gpu.py."""
import numpy as np


def joint_counts(x, y, edges_x, edges_y):
    """(counts int64 [bx, by], outside int64 [3]) of the float32 series x, y against the fp64 edge tables.  np.histogramdd drops
    what is outside explicit edges and NaN, so every value goes through it; the outside counters are
    [x outside and no NaN, x inside and y outside, a NaN in either]."""
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    ex, ey = np.asarray(edges_x, dtype=np.float64), np.asarray(edges_y, dtype=np.float64)
    nan = np.isnan(x) | np.isnan(y)
    keep = ~nan
    counts = np.histogramdd(np.stack([x[keep], y[keep]], axis=1), bins=(ex, ey))[0]
    assert (counts == np.floor(counts)).all()
    with np.errstate(invalid="ignore"):
        x_out = keep & ((x < ex[0]) | (x > ex[-1]))
        y_out = keep & ~x_out & ((y < ey[0]) | (y > ey[-1]))
    return counts.astype(np.int64), np.array([x_out.sum(), y_out.sum(), nan.sum()], dtype=np.int64)


def joint_pairs(X, pairs, edges_x, edges_y):
    """(counts [P, bx, by], outside [P, 3]) of the column pairs of X [T, C] against per-pair tables [P, bx + 1], [P, by + 1]."""
    out = [joint_counts(X[:, i], X[:, j], edges_x[p], edges_y[p]) for p, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2))]
    bx, by = np.asarray(edges_x).shape[1] - 1, np.asarray(edges_y).shape[1] - 1
    if not out:
        return np.zeros((0, bx, by), dtype=np.int64), np.zeros((0, 3), dtype=np.int64)
    return np.stack([c for c, _ in out]), np.stack([o for _, o in out])


def linspace_tables(lo, hi, bins, n_pairs):
    """[n_pairs, bins + 1]: np.linspace(lo, hi, bins + 1) for every pair (scalars or per-pair arrays)."""
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (n_pairs,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (n_pairs,))
    return np.stack([np.linspace(l, h, bins + 1) for l, h in zip(lo, hi)]) if n_pairs else np.zeros((0, bins + 1))


def planted(lo, hi, bins, rng, n):
    """n float32 values: the float32 nearest to every edge of np.linspace(lo, hi, bins + 1) and its two float32 neighbours (as many
    as n allows, shuffled), then uniform draws over a slightly wider interval, so that some fall outside."""
    e = np.linspace(lo, hi, bins + 1).astype(np.float32)
    inf = np.float32(np.inf)
    on = np.concatenate([e, np.nextafter(e, -inf), np.nextafter(e, inf)])
    rng.shuffle(on)
    free = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), max(n - len(on), 0)).astype(np.float32)
    out = np.concatenate([on[:n], free]).astype(np.float32)
    rng.shuffle(out)
    return out


def trajectory(T, seed, states=4):
    """[T, 2] float32, time-ordered like MD frames: a chain that dwells in one of `states` wells for long stretches."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-2, 2, size=(states, 2))
    jumps = rng.random(T) < 0.002
    state = np.cumsum(jumps) % states
    return (centres[state] + 0.05 * rng.normal(size=(T, 2))).astype(np.float32)
