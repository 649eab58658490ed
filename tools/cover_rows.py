#!/usr/bin/env python3
"""Grows the pairwise cover of the decode chain's options that tests/cover_cases.py commits as a literal table (DESIGN.md section 2,
"The options meet").

    python tools/cover_rows.py            # prints the rows as the tuples of cover_cases.ROWS

The factors, their values and the constraints are cover_cases.FACTORS / cover_cases.allowed: add a factor or a value there, run this,
and paste the rows over the table.  Nothing here draws from `random` (its choice / shuffle are not stable across Python versions): the
candidate orders come from a 64-bit LCG, so the same factors give the same table everywhere.

The method is the greedy one of AETG: a new row is started from the uncovered pair with the most uncovered pairs behind its values,
the remaining factors are filled in one of CANDIDATES orders, each with the value that covers the most pairs still uncovered, and the
best candidate row is kept.  Rows the link cannot carry (cover_cases.carried) are not grown.  A last pass drops every row the cover
holds without, so that each row left is needed (tests/test_cover_cpu.py asserts both)."""
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import cover_cases as cc  # noqa: E402

CANDIDATES = 60


class Lcg:
    def __init__(self, seed):
        self.s = seed & (2 ** 64 - 1)

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.s >> 33) % n

    def order(self, items):
        items = list(items)
        for i in range(len(items) - 1, 0, -1):
            j = self.below(i + 1)
            items[i], items[j] = items[j], items[i]
        return items


def pairs_of(row):
    return {((i, row[i]), (j, row[j])) for i, j in itertools.combinations(range(len(row)), 2)}


def completes(partial):
    """a partial row {factor index: value} can still be completed to a row that is allowed and carried"""
    free = [i for i in range(len(cc.FACTORS)) if i not in partial]
    # the rules read a few factors only: try their values, leave the others at their first
    touched = [i for i in free if cc.NAMES[i] in cc.CONSTRAINED + cc.LINK_FACTORS]
    base = {i: cc.FACTORS[i][1][0] for i in free}
    for combo in itertools.product(*[cc.FACTORS[i][1] for i in touched]):
        full = {**base, **partial, **dict(zip(touched, combo))}
        row = tuple(full[i] for i in range(len(cc.FACTORS)))
        if cc.allowed(row) and cc.carried(row):
            return True
    return False


def grow():
    todo = set(cc.allowed_pairs())
    rng = Lcg(2024)
    n = len(cc.FACTORS)
    rows = []
    while todo:
        weight = {}
        for a, b in todo:
            weight[a] = weight.get(a, 0) + 1
            weight[b] = weight.get(b, 0) + 1
        seed_pair = max(sorted(todo), key=lambda p: weight[p[0]] + weight[p[1]])
        best, best_gain = None, -1
        for _ in range(CANDIDATES):
            partial = {seed_pair[0][0]: seed_pair[0][1], seed_pair[1][0]: seed_pair[1][1]}
            for i in rng.order(k for k in range(n) if k not in partial):
                scored = []
                for v in cc.FACTORS[i][1]:
                    trial = {**partial, i: v}
                    if not completes(trial):
                        continue
                    gain = sum(1 for j, w in partial.items() if (min((i, v), (j, w)), max((i, v), (j, w))) in todo)
                    scored.append((gain, v))
                top = max(g for g, _ in scored)
                ties = [v for g, v in scored if g == top]
                partial[i] = ties[rng.below(len(ties))]
            row = tuple(partial[i] for i in range(n))
            assert cc.allowed(row) and cc.carried(row)
            gain = len(pairs_of(row) & todo)
            if gain > best_gain:
                best, best_gain = row, gain
        assert best_gain > 0
        rows.append(best)
        todo -= pairs_of(best)
    # drop what the cover holds without, last grown first
    want = set(cc.allowed_pairs())
    for r in reversed(list(rows)):
        rest = [x for x in rows if x is not r]
        if want <= set().union(*[pairs_of(x) for x in rest]):
            rows = rest
    return rows


if __name__ == "__main__":
    rows = grow()
    print(f"# {len(cc.allowed_pairs())} allowed pairs in {len(rows)} rows")
    for r in sorted(rows):
        print(f"    {r!r},")
