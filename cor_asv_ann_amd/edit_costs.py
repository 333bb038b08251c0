"""Weighted edit costs for the vote, the confusion network and the risk (include/cor_asv_ann_hip.h,
casv_edit_costs): what an insertion or deletion and a substitution cost, and a key per character under which two different
characters count as near.  The device compares characters twice -- as themselves, which is what a vote class is made of, and by
their keys, which only the alignment's costs read -- so 'ſ' and 's' stay two classes of one column and still cost nothing (or half
an edit) against each other."""
import unicodedata

import numpy as np

from . import metrics

COST_MAX = 255          # EDIT_COST_MAX of csrc/common.h
MAX_L = 2048            # CONSENSUS_COSTED_MAX_L: the costed calls' longest candidate


class EditCosts(object):
    """gap: an insertion or a deletion, 1..255.  sub: a substitution, near: a substitution between two different characters of
    equal key, 0 <= near <= sub <= 255.  unit: what one full edit costs, 1..255 -- the normalised risk and the training cost
    divide by unit x length; None: sub.  key: None (no two characters are near), a dict code point -> int (a code point it lacks
    is its own key, apart from every value of the dict) or a callable on a one-character string that returns something hashable;
    a callable is asked once per distinct code point and its answers are kept.  ValueError for anything else."""

    def __init__(self, gap=1, sub=1, near=1, key=None, unit=None, name=None):
        for what, value in (('gap', gap), ('sub', sub), ('near', near)) + ((('unit', unit),) if unit is not None else ()):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
                raise ValueError('%s=%r: an integer' % (what, value))
        if not 1 <= gap <= COST_MAX:
            raise ValueError('gap=%d outside 1..%d' % (gap, COST_MAX))
        if not 0 <= sub <= COST_MAX:
            raise ValueError('sub=%d outside 0..%d' % (sub, COST_MAX))
        if not 0 <= near <= sub:
            raise ValueError('near=%d outside 0..sub=%d' % (near, sub))
        if unit is None:
            if sub < 1:
                raise ValueError('sub=0 names no cost of a full edit: give unit')
            unit = sub
        if not 1 <= unit <= COST_MAX:
            raise ValueError('unit=%d outside 1..%d' % (unit, COST_MAX))
        if key is not None and not isinstance(key, dict) and not callable(key):
            raise ValueError('key=%r: None, a dict code point -> int or a callable on a character' % (key,))
        self.gap, self.sub, self.near, self.unit = int(gap), int(sub), int(near), int(unit)
        self.key = key
        self.name = name                # of a preset: what a training run records in place of the key
        self._memo = {}

    def __repr__(self):
        return 'EditCosts(gap=%d, sub=%d, near=%d, unit=%d, key=%s)' % (
            self.gap, self.sub, self.near, self.unit, self.name or ('None' if self.key is None else '...'))

    def as_tuple(self):
        """(gap, sub, near, unit): the fields of casv_edit_costs."""
        return self.gap, self.sub, self.near, self.unit

    def key_of(self, point):
        """The key of one code point, before the ids: any hashable."""
        point = int(point)
        if point not in self._memo:
            if isinstance(self.key, dict):
                self._memo[point] = ('key', self.key[point]) if point in self.key else ('self', point)
            else:
                self._memo[point] = self.key(chr(point))
        return self._memo[point]

    def keys_of(self, points):
        """The key arrays beside `points` -- per source a list of int32 arrays of code points, as `Sequence2Sequence._vote_inputs`
        makes them -- in the same nesting: per code point a dense int32 id of its key, numbered per call in order of first
        appearance (keys are compared for equality only).  None without a key."""
        if self.key is None:
            return None
        ids, table = {}, {}
        out = []
        for cands in points:
            for p in cands:
                for x in np.unique(p).tolist():
                    if x not in table:
                        table[x] = ids.setdefault(self.key_of(x), len(ids))
            out.append([np.array([table[x] for x in p.tolist()], np.int32) for p in cands])
        return out

    def settings(self):
        """What a training run records: the costs and the preset's name.  ValueError for a key that has no name."""
        if self.key is not None and self.name is None:
            raise ValueError('risk_costs: only None, EditCosts without a key or a preset (historic_latin, graded) can be recorded')
        return {'gap': self.gap, 'sub': self.sub, 'near': self.near, 'unit': self.unit, 'key': self.name}

    # -------------------------------------------------------------------------------------------------------------- the presets
    @classmethod
    def historic_latin(cls):
        """gap 1, sub 1, near 0, and as key the lowest single-code-point member of the character's class in
        `metrics.L1_EQUIVALENCES`, else the character itself: ſ/s, ꝛ/r, the quote and dash families and the rest of level 1 of
        the 'historic_latin' normalisation cost nothing against each other.  The classes' members of more than one code point
        (a + U+0308 for ä ...) and the level-2 replacements (ligatures, private-use code points) are rewriting of strings, which
        costs per character cannot express: apply `metrics.normalize_text(line, 'historic_latin')` to the lines first where
        they matter."""
        lowest = {}
        for members in metrics.L1_EQUIVALENCES:
            single = sorted(m for m in members if len(m) == 1)
            for m in single:
                lowest[m] = single[0]
        return cls(1, 1, 0, key=lambda char: lowest.get(char, char), name='historic_latin')

    @classmethod
    def graded(cls):
        """gap 2, sub 2, near 1, and as key the case-folded first code point of the character's NFD form where that is a single
        character (else the character itself): a difference in case or in diacritics only costs half an edit."""
        def key(char):
            base = unicodedata.normalize('NFD', char)[:1].casefold()
            return base if len(base) == 1 else char
        return cls(2, 2, 1, key=key, name='graded')
