"""The no-speech kernel alone (spt_debug_no_speech: dec_no_speech of k_sample.hip) against the float64
reference of tests/nospeech_ref.py on its crafted rows: every V of the table, nosp at the row's ends
and on both sides of a chunk boundary, at B = 1, 5 and 64.  Each row is within its own bar, a row's bits
in a batch are its bits alone, and two runs give the same bits."""
import math

import numpy as np
import pytest

from tests import nospeech_ref as R

pytestmark = pytest.mark.gpu

def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("pos", ["first", "last", "chunk_end", "chunk_begin"])
@pytest.mark.parametrize("V", R.VOCABS)
def test_rows_against_float64(V, pos):
    from spittle_amd import nospeech_debug as D
    nosp = R.positions(V)[pos]
    names, lg = R.rows(V, nosp)                       # [10][V + 5], the pad holds +1e30 and NaN
    n = len(names)
    alone = np.concatenate([D.no_speech(lg[i:i + 1], nosp, n_vocab=V) for i in range(n)])   # B = 1
    for i, name in enumerate(names):
        want = R.prob(lg[i, :V], nosp)
        if math.isnan(want):
            assert math.isnan(alone[i]), (name, alone[i])
            continue
        b = R.bar(lg[i, :V], nosp)
        err = abs(float(alone[i]) - want)
        print(f"V={V} {pos} {name}: p={want:.9g} err={err:.3g} bar={b:.3g} err/bar={err / b:.3f}")
        assert err <= b, (name, float(alone[i]), want, b)
    for B in (5, 64):                                 # a row's bits in a batch are its bits alone
        pick = [(3 * k + B) % n for k in range(B)]
        got = D.no_speech(lg[pick], nosp, n_vocab=V)
        assert np.array_equal(_bits(got), _bits(alone[pick])), (B, got, alone[pick])
        assert np.array_equal(_bits(D.no_speech(lg[pick], nosp, n_vocab=V)), _bits(got)), B   # two runs


def test_worst_fraction_of_the_bar():
    """the largest error over every crafted row as a fraction of its bar, computed here from launches of
    its own (one batch per (V, nosp)); printed for DESIGN 4.6"""
    from spittle_amd import nospeech_debug as D
    worst, n = 0.0, 0
    for V in R.VOCABS:
        for pos, nosp in R.positions(V).items():
            names, lg = R.rows(V, nosp)
            got = D.no_speech(lg, nosp, n_vocab=V)
            for i in range(len(names)):
                want = R.prob(lg[i, :V], nosp)
                if not math.isnan(want):
                    worst = max(worst, abs(float(got[i]) - want) / R.bar(lg[i, :V], nosp))
                    n += 1
    print(f"largest err / bar over {n} finite kernel cases: {worst:.3f}")
    assert n == 8 * 4 * len(R.VOCABS) and worst <= 1.0
