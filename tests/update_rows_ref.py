"""The numpy twin of ggms_update_rows (include/ggms.h): the two rules with every intermediate a numpy float32.

numpy rounds each float32 operation to nearest even, keeps subnormals, has correctly rounded divide and square root and
no FMA: the kernel must give the same bits.  `update_rows` applies a rule to a table in place the way the entry point
does (distinct nodes, EMPTY entries skipped, a count below the bound); `rule_f64` is the same formula in float64, the
yardstick the twin itself is held against."""
import numpy as np

SGD, ADAGRAD = 0, 1
EMPTY = 0xFFFFFFFF
F = np.float32


def sgd(w, g, lr):
    """w' = fl(w - fl(lr * g)) on float32 arrays."""
    w, g = np.asarray(w, dtype=F), np.asarray(g, dtype=F)
    with np.errstate(all="ignore"):
        step = (F(lr) * g).astype(F)
        return (w - step).astype(F)


def adagrad(w, s, g, lr, eps):
    """(w', s'): s' = fl(s + fl(g * g)); w' = fl(w - fl(fl(lr * g) / fl(fl(sqrt(s')) + eps)))."""
    w, s, g = np.asarray(w, dtype=F), np.asarray(s, dtype=F), np.asarray(g, dtype=F)
    with np.errstate(all="ignore"):
        gg = (g * g).astype(F)
        s2 = (s + gg).astype(F)
        num = (F(lr) * g).astype(F)
        den = (np.sqrt(s2).astype(F) + F(eps)).astype(F)
        step = (num / den).astype(F)
        return (w - step).astype(F), s2


def rule_f64(rule, w, s, g, lr, eps):
    """The rules in float64 on the float32 inputs: (w', s', step)."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    lr, eps = float(F(lr)), float(F(eps))
    with np.errstate(all="ignore"):
        if rule == SGD:
            step = lr * g
            return w - step, None, step
        s2 = np.asarray(s, dtype=np.float64) + g * g
        step = lr * g / (np.sqrt(s2) + eps)
        return w - step, s2, step


def update_rows(table, state, nodes, grad, rule, lr, eps=1e-10, count=None):
    """ggms_update_rows on numpy arrays, in place: table / state (rows, dim) float32, nodes uint32 ids (pairwise
    distinct but for EMPTY), grad (>= count, dim) float32."""
    nodes = np.asarray(nodes).astype(np.int64) & 0xFFFFFFFF
    n = nodes.size if count is None else min(int(count), nodes.size)
    keep = np.flatnonzero(nodes[:n] != EMPTY)
    v = nodes[keep]
    assert np.unique(v).size == v.size, "update_rows: the nodes of a call are pairwise distinct"
    g = np.asarray(grad, dtype=F).reshape(-1, table.shape[1])[keep]
    if rule == SGD:
        table[v] = sgd(table[v], g, lr)
    else:
        table[v], state[v] = adagrad(table[v], state[v], g, lr, eps)
    return table
