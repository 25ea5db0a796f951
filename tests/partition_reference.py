"""Pure-Python statement of the partition rule of a multi-device handle (test comparator for csrc/pfc_partition.h and, on the
GPU, for pfc_last_shard_bounds).  Python floats are IEEE doubles and every sum is taken in the order the library takes it, so
bounds and keep decisions are compared for equality.  Test infrastructure: not part of the product package."""


def cost_leaves(n_leaf_1, n_leaf_2):
    """Cost of an item the first time its list is seen: the leaf-count product of its two meshes."""
    return 64.0 + 0.02 * float(n_leaf_1) * float(n_leaf_2)


def cost_counters(node_tests, candidates):
    """Cost of an item from counters 0 and 1 of its row in the previous evaluation of the same list."""
    return 64.0 + float(node_tests) + 4.0 * float(candidates)


def k_use(n, K, min_items):
    """Shards that take part: clamp(n / max(min_items, 1), 1, K)."""
    return max(1, min(K, n // max(min_items, 1)))


def _total(cost):
    total = 0.0
    for c in cost:
        total += c
    return total


def shard_costs(cost, bound, ku):
    out = []
    for k in range(ku):
        c = 0.0
        for i in range(bound[k], bound[k + 1]):
            c += cost[i]
        out.append(c)
    return out


def keeps(cost, bound, ku):
    """The 15 % rule: the most loaded shard times the shards used is at most 1.15 times the total."""
    return max([0.0] + shard_costs(cost, bound, ku)) * ku <= 1.15 * _total(cost)


def cut(cost, ku, K):
    """bound[0..K]: boundary k goes in front of the first item whose half would cross k / ku of the total, then is clamped so
    that every used shard has an item; bound[k] = n for k >= ku."""
    n = len(cost)
    total = _total(cost)
    bound = [0] * (K + 1)
    acc, i = 0.0, 0
    for k in range(1, ku):
        target = total * float(k) / float(ku)
        while i < n and acc + 0.5 * cost[i] < target:
            acc += cost[i]
            i += 1
        b = min(max(i, bound[k - 1] + 1), n - (ku - k))
        while i < b:
            acc += cost[i]
            i += 1
        bound[k] = b
    for k in range(ku, K + 1):
        bound[k] = n
    return bound


class Partitioner:
    """What multi_partition does with the three functions over successive evaluations on one handle: the previous ranges are
    kept while the item list is the same, as many shards are used and keeps() holds under the new costs."""

    def __init__(self, K, min_items=8):
        self.K, self.min_items = K, min_items
        self.bound, self.n_used, self.key = None, 1, None

    def set_min_items(self, v):
        self.min_items = max(int(v), 1)
        self.key = None

    def step(self, key, cost):
        """key: what identifies the item list (n, the ids or None, the entry-point family); cost: one float per item.
        Returns (bound[0..n_used], kept)."""
        n = len(cost)
        ku = k_use(n, self.K, self.min_items)
        same = self.key is not None and self.key == key
        kept = same and self.n_used == ku and keeps(cost, self.bound, ku)
        if not kept:
            self.bound, self.n_used, self.key = cut(cost, ku, self.K), ku, key
        return self.bound[:self.n_used + 1], kept
