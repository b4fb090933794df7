"""numpy restatement of routing packed rows: a thin loop over ``mix_reference``.

``routes`` holds O sequences of S entries, an int gain or None.  With inc_o = [i : routes[o][i] is not None], output o is

    np_mix([sources[i] for i in inc_o], gains=[routes[o][i] for i in inc_o], active=active[inc_o])

and, where inc_o is empty, the slot np_mix gives when every source is inactive.  ``route_budget`` is that loop on rows that are
unpacked already (np_mix's two lines, so that a test unpacks every source once); ``np_route`` is the rows-to-rows form.
"""

import numpy as np

from mix_reference import mix_budget
from pack_reference import np_unpack
from pack_rows_reference import np_rows_from_codes


def heard(route):
    return [i for i, g in enumerate(route) if g is not None]


def mix_minus(S, gains=None):
    """The table of a bridge: output o hears every source but o, source i at gains[i]."""
    gains = [0] * S if gains is None else list(gains)
    return [[None if i == o else gains[i] for i in range(S)] for o in range(S)]


def route_budget(rows, off, R, routes, active=None):
    """rows = [(codes, sf), ...] -> per output what mix_budget returns: [(codes, sf, offset, row_bits_out), ...]."""
    outs = []
    active = None if active is None else np.asarray(active)
    for route in routes:
        inc = heard(route)
        assert len(route) == len(rows)
        if inc:
            outs.append(mix_budget([rows[i] for i in inc], off, R, [route[i] for i in inc], None if active is None else active[inc]))
        else:                                                               # nothing heard: a mix of inactive rows
            B, F, _, C = rows[0][0].shape
            outs.append(mix_budget(rows[:1], off, R, [0], np.zeros((1, B, F, C), np.uint8)))
    return outs


def route_rows(rows, off, R, routes, active=None):
    """... -> (data' [O, rows row_bytes], index' [B, F, C], fits' [O, B, F, C], offset [O, B, F, C], row_bits_out [O, B, F, C])."""
    outs = [np_rows_from_codes(rc, rs, bits, off, R) + (offset, bits) for rc, rs, offset, bits in route_budget(rows, off, R, routes, active)]
    for o in outs[1:]:
        np.testing.assert_array_equal(o[1], outs[0][1])                      # one index for every output
    return (np.stack([o[0] for o in outs]), outs[0][1], np.stack([o[2] for o in outs]), np.stack([o[3] for o in outs]),
            np.stack([o[4] for o in outs]))


def np_route(sources, off, N, R, routes, active=None):
    """What route_packed_rows stores at the budget R: sources = [(data, index [B, F, C]), ...]."""
    return route_rows([np_unpack(data, index, off, N) for data, index in sources], off, R, routes, active)
