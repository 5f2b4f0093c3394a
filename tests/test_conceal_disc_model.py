"""The disc tier's conceal mode, CPU side: the damaged tracks tests/test_gpu_conceal_disc.py reads, put to the rule's
model (tests/conceal_model.py).  What is asserted here is what the GPU cases rely on: the damage shows as the spans it
should, every span is far shorter than 65 536 frames (the gap's wrap term is 0, so a reader that saw the track in pieces
would agree with one that saw it whole), and the composed track is as long as the clean one."""
import numpy as np
import pytest

from tests import conceal_model as cm
from tests import disc_damage as dd
from tests.test_conceal_model import make_stream

KINDS = [(1, 0), (2, "DISC|CHAINED"), (1, "CHAINED")]
# name -> (damage, span count): two pairs of lost sectors and a flipped byte; a hole longer than a 64-sector window
# (sectors are lost in even numbers: a sector carries an odd number of MLP bytes, and access units start at even offsets)
DAMAGES = {
    "scattered": (dict(lost=(63, 64, 200, 201), flips=((150, 1000, 0x10),)), 3),
    "long_hole": (dict(lost=tuple(range(100, 170))), 1),
}
N_AUS, FRAMES = 800, 64000

_CACHE = {}


def stream_of(pkg, S, feat):
    key = ("stream", S, feat)
    if key not in _CACHE:
        _CACHE[key] = make_stream(pkg, S, feat, seed=21, n_aus=N_AUS)
    return _CACHE[key]


def model_of(pkg, oracle, S, feat, name):
    """-> (sectors, D, composed PCM [6, frames], spans) of one damaged track; cached: every reader of a case shares it"""
    key = (S, feat, name)
    if key not in _CACHE:
        b, frames, rpa = stream_of(pkg, S, feat)
        sectors, D = dd.damaged_track(pkg.disc, b, **DAMAGES[name][0])
        pcm, spans = cm.conceal(D, 6, rpa, oracle)
        _CACHE[key] = (sectors, D, pcm, spans)
    return _CACHE[key]


@pytest.mark.parametrize("name", sorted(DAMAGES))
@pytest.mark.parametrize("S,feat", KINDS)
def test_damaged_tracks_sit_inside_the_unwrapped_gap(pkg, oracle, S, feat, name):
    b, frames, rpa = stream_of(pkg, S, feat)
    assert frames == FRAMES
    sectors, D, pcm, spans = model_of(pkg, oracle, S, feat, name)
    assert 387 <= len(sectors) <= 414
    n_spans = DAMAGES[name][1]
    print("spans:", spans)
    assert len(spans) == n_spans, spans
    assert all(0 < s[1] < 65536 and s[4] == 0 for s in spans), spans
    # the gaps are the input timing's alone (w = 0): the composed track is as long as the clean one
    assert pcm.shape == (6, FRAMES)
    # ... and outside the spans it is the clean track's PCM wherever a kept range starts with the clean decoder's state:
    # the first range always does
    want, r, st = oracle.decode(b, 6, frames)
    assert st == 0 and np.array_equal(pcm[:, :spans[0][0]], want[:, :spans[0][0]])


def test_track_stream_follows_the_end_of_track_rule(pkg):
    """disc_damage.track_stream on an undamaged two-track title: the tracks' streams partition the title's stream at the
    first major sync at or behind the second track's first payload byte"""
    b, frames, rpa = stream_of(pkg, 1, 0)
    sectors, bodies = dd.damaged_sectors(pkg.disc, b)
    assert [len(s) for s in sectors] == [2048] * len(sectors) and b"".join(bodies) == bytes(b)
    cut = 200
    d1 = dd.track_stream(bodies, 0, cut - 1)
    d2 = dd.track_stream(bodies, cut, len(bodies) - 1)
    assert np.array_equal(np.concatenate([d1, d2]), b)
    assert len(d1) >= cut * dd.BODY and bytes(d2[4:8]) == dd.PATTERN
    assert dd.find_sync(bytes(b), cut * dd.BODY) == len(d1)
