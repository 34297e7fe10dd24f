"""The float32 rasteriser model's own distance from its float64 variant, on the fixed scenes the GPU tests use (both sides
are models: tests/raster_ref.py; nothing random).  Written to tests/golden/floors/raster.json by running this file;
tests/test_raster_cpu.py holds the committed file against a fresh measurement.

Per scene: the covered samples, the samples whose winner differs between the two models and how many of those the
float64 model shows to be depth near-ties, the largest depth difference where the winners agree, and for lit records the
samples whose 8-bit colour differs at all and by how many levels at most, and the textured samples for which float64
arithmetic alone would pick another texel (sample centres on texel edges: the float64 variant takes the float32 choice).

A near-tie: the float64 depths of the two winners differ by at most TIE.  The float32 depth of a candidate carries three
conversions, three divisions for the weights, one division per corner depth, three products and two sums, each within
half an ulp of a value of at most 1 (the weights of a covered sample and the accepted depths lie in [0, 1]): within
7 * 2^-24 of the float64 value, so two candidates can change places only when their float64 depths are within
14 * 2^-24; TIE = 16 * 2^-24."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import raster_ref as RR  # noqa: E402
import raster_scenes as SC  # noqa: E402

TIE = 16 * 2.0 ** -24
PATH = os.path.join(HERE, 'golden', 'floors', 'raster.json')
LIGHT = dict(ambient=0.15, diffuse=0.85, background=(0.7, 0.8, 1.0))


def scenes():
    c = SC.cases()
    return {'perspective': c['perspective'], 'interpenetrating': c['interpenetrating'], 'both_paths': c['both_paths'],
            'ssaa3': c['ssaa3'], 'shading': SC.shading_scene(), 'texel_ties': SC.texel_ties()}


def compare(sc):
    a, b = SC.model(sc, np.float32, **LIGHT), SC.model(sc, np.float64, **LIGHT)
    ia, ib = a['ids'].reshape(-1), b['ids'].reshape(-1)
    assert np.array_equal(a['cand']['pix'], b['cand']['pix'])            # the same coverage: the candidates line up
    differ = np.nonzero(ia != ib)[0]
    ties = 0
    for p in differ:
        da = b['d'][a['win'][p]] if a['win'][p] >= 0 else np.inf          # the float64 depth of each model's winner
        db = b['d'][b['win'][p]] if b['win'][p] >= 0 else np.inf
        ties += bool(abs(da - db) <= TIE)
    same = (ia == ib) & (ia >= 0)
    lit = np.zeros(len(ia), bool)
    recs = SC.recs(sc)
    for r, rec in enumerate(recs):
        if not rec.flags & RR.UNLIT:
            lit |= same & (a['cand']['rec'][np.maximum(a['win'], 0)] == r)
    lv = np.abs(a['samples'].reshape(-1, 3).astype(int) - b['samples'].reshape(-1, 3).astype(int)).max(1)
    exact = same & ~lit
    own = SC.model(sc, np.float64, own_texels=True, **LIGHT)['texel']         # the texel float64 would pick by itself
    textured = same & (a['texel'][:, 0] >= 0)
    return dict(covered=int(np.sum(ia >= 0)), winner_differs=int(len(differ)), differing_winners_that_are_near_ties=int(ties),
                max_depth_difference=float(np.abs(a['depth'].reshape(-1)[same].astype(np.float64) - b['depth'].reshape(-1)[same]).max(initial=0)),
                lit_samples=int(lit.sum()), lit_samples_that_differ=int(np.sum(lv[lit] > 0)),
                max_lit_level_error_f32=int(lv[lit].max(initial=0)), unlit_samples_that_differ=int(np.sum(lv[exact] > 0)),
                textured_samples=int(textured.sum()), texel_choice_differs=int(np.sum(np.any(a['texel'] != own, 1) & textured)))


def measure():
    return dict(tie=TIE, scenes={name: compare(sc) for name, sc in scenes().items()})


if __name__ == '__main__':
    out = measure()
    with open(PATH, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))
