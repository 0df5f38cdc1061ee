"""The per-item entry points — `spf_sample_extract_l1_each_*`, `spf_glwe_mul_xn_each_*`, `spf_glwe_keyswitch_each_*`,
`spf_glwe_automorphism_each_*` in their `_batch`, `_dev` and group forms: ONE call over items whose parameters differ.

Two rigs of tests/glwe_keyswitch_cases.py: DEFAULT_128 under 6 x 7 keys (the hand-written `glwe_ks_each_kernel`, four units per
workgroup) and `N16`, a generic context (`generic_glwe_ks_each_kernel`, one); both also hold a key at OTHER_RADIX, which never
shares a launch with the others.  B = 9 items (the case's five GLWEs, in rotation) whose parameters form runs of 1, 3 and 5, given
interleaved and not sorted: the four-unit workgroup sees a run shorter than a workgroup, a ragged run and a run across two
workgroups.  Every comparison is word for word — against the oracle, and against the single-parameter entry point called once per
distinct parameter.  There is no tolerance in this file."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import oracle as O
import spf_amd
from spf_amd import SpfError
from tests import glwe_keyswitch_cases as KC
from tests import glwe_keyswitch_graph_cases as G

pytestmark = pytest.mark.gpu
U = np.uint64
INVALID, NO_KEY = 1, 3
TUNED, SMALL = G.TUNED, "N16"
A, B2, OTHER, THIRD, EMPTY = G.A2B_SLOT, G.SECOND_SLOT, G.OTHER_SLOT, 7, G.EMPTY_SLOT
B = 9
# positions of the runs of 1, 3 and 5 among the nine items: p[0] once, p[1] three times, p[2] five times
PATTERN = [2, 1, 2, 0, 2, 1, 2, 1, 2]
SENTINEL = U(0xA5A5_5A5A_C3C3_3C3C)
EACH_KERNEL = {True: "glwe_ks_each_kernel", False: "generic_glwe_ks_each_kernel"}


def spread(three):
    assert sorted(PATTERN.count(i) for i in range(3)) == [1, 3, 5]
    return [three[i] for i in PATTERN]


def items(c):
    return np.ascontiguousarray(np.stack([c.x[i % KC.ITEMS] for i in range(B)]))


def slot_keys(c):
    keys = dict(G.slot_keys(c))
    keys[OTHER] = KC.other_radix_key(c) + (KC.OTHER_RADIX,)
    keys[THIRD] = (c.ksk, c.ksk_fft, (c.P.tr_radix_log, c.P.tr_count))
    return keys


def load_keys(eng, c):
    G.load_keys(eng, c)
    for slot in (OTHER, THIRD):
        words, _, (lg, cnt) = slot_keys(c)[slot]
        eng.load_glwe_keyswitch_key_std(slot, words, lg, cnt)


def cases(shape):
    """(id, operation, the nine parameters)"""
    c = KC.case(shape)
    N, log_n = c.P.N, KC.log2n(c.P)
    return [("keyswitch-one-shape", "ks", spread([THIRD, B2, A])),
            ("keyswitch-two-slots", "ks", [A, B2, A, B2, B2, A, A, B2, A]),
            ("keyswitch-another-shape", "ks", spread([OTHER, B2, A])),
            ("automorphism", "au", spread([log_n, 2, 1])),
            ("sample-extract", "se", spread([N - 1, 1, 0])),
            ("mul-xn", "mx", spread([N + 77, 2 * N - 1, 0]))]


DRAWN = [pytest.param(shape, op, tuple(params), id=f"{shape}-{name}") for shape in (TUNED, SMALL) for name, op, params in cases(shape)]


@functools.lru_cache(maxsize=None)
def oracle_row(shape, op, param, item):
    """the oracle's words of one operation on item `item` of the case, computed once in a process"""
    c = KC.case(shape)
    P, x = c.P, c.x[item]
    if op == "se":
        out = O.sample_extract(x.reshape(-1), param, P.N, P.k)
    elif op == "mx":
        out = O.glwe_mul_xn(x.reshape(-1), param, P.N, P.k)
    elif op == "ks":
        _, fft, radix = slot_keys(c)[param]
        out = KC.oracle_keyswitch(P, x, fft, radix)
    else:
        out = KC.oracle_round(c, x, param)
    out = np.array(out, dtype=U).reshape(-1)
    out.setflags(write=False)
    return out


def want(shape, op, params):
    return np.stack([oracle_row(shape, op, int(p), i % KC.ITEMS) for i, p in enumerate(params)])


def each(eng, op, x, params, out=None):
    if op == "se":
        return eng.sample_extract_l1_each(x, params, out)
    if op == "mx":
        return eng.glwe_mul_xn_each(x, params, out)
    if op == "ks":
        return eng.glwe_keyswitch_each(params, x, out)
    return eng.glwe_automorphism_each(params, x, out)


def each_dev(eng, op, stream, n, d_in, params, d_out):
    if op == "se":
        return eng.sample_extract_l1_each_dev(stream, n, d_in, params, d_out)
    if op == "mx":
        return eng.glwe_mul_xn_each_dev(stream, n, d_in, params, d_out)
    if op == "ks":
        return eng.glwe_keyswitch_each_dev(stream, params, n, d_in, d_out)
    return eng.glwe_automorphism_each_dev(stream, params, n, d_in, d_out)


def single(eng, op, x, param):
    """the single-parameter entry point this replaces"""
    if op == "se":
        return eng.sample_extract_l1(x, param)
    if op == "mx":
        return eng.glwe_mul_xn(x, param)
    if op == "ks":
        return eng.glwe_keyswitch(param, x)
    return eng.glwe_automorphism(param, x)


def out_words(c, op):
    return c.P.k * c.P.N + 1 if op == "se" else (c.P.k + 1) * c.P.N


@pytest.fixture(scope="module")
def rigs():
    """shape -> (case, engine with every key), made when a test first asks"""
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            eng = spf_amd.Engine(G.engine_params(c.P))
            load_keys(eng, c)
            made[shape] = (c, eng)
        return made[shape]

    yield get
    gc.collect()
    for _, eng in made.values():
        eng.close()


@pytest.fixture(scope="module")
def groups():
    """shape -> a group over [0, 0] with every key, made when a test first asks"""
    made = {}

    def get(shape):
        if shape not in made:
            c = KC.case(shape)
            made[shape] = spf_amd.Group(G.engine_params(c.P), devices=[0, 0])
            load_keys(made[shape], c)
        return made[shape]

    yield get
    gc.collect()
    for grp in made.values():
        grp.close()


@pytest.mark.parametrize("shape,op,params", DRAWN)
def test_one_call_equals_the_oracle_and_one_call_per_parameter(rigs, shape, op, params):
    c, eng = rigs(shape)
    x, w = items(c), out_words(c, op)
    params = list(params)
    # sentinel rows in front of and behind the output block
    block = np.full((B + 2, w), SENTINEL, dtype=U)
    got = each(eng, op, x, params, block[1:B + 1])
    assert np.all(block[0] == SENTINEL) and np.all(block[B + 1] == SENTINEL), (shape, op)
    assert G.same_words(x, items(c))                                              # the inputs are the caller's: untouched
    expect = want(shape, op, params)
    for i in range(B):
        assert G.same_words(got[i], expect[i]), (shape, op, i, params[i])
    if op in ("ks", "au"):
        # one launch per radix shape, in the order the shapes first appear: the OTHER_RADIX slot stands at position 3, behind the
        # trace-radix slots, so where it is named the generic kernel ran last
        assert eng.last_glwe_keyswitch_kernel() == EACH_KERNEL[shape == TUNED and not (op == "ks" and OTHER in params)], (shape, op)
    for p in sorted(set(params)):                                                  # the existing entry point, once per distinct parameter
        at = [i for i in range(B) if params[i] == p]
        alone = single(eng, op, x[at], p).reshape(len(at), -1)
        for j, i in enumerate(at):
            assert G.same_words(got[i], alone[j]), (shape, op, i, p)


@pytest.mark.parametrize("shape,op,params", DRAWN)
def test_batch_dev_and_group_forms_agree(rigs, groups, shape, op, params):
    c, eng = rigs(shape)
    x, w = items(c), out_words(c, op)
    params = list(params)
    by_batch = each(eng, op, x, params).reshape(B, w)
    # _dev on the null stream: a block with a sentinel row on either side
    d_in, d_out = eng.device_alloc(x.nbytes), eng.device_alloc((B + 2) * w * 8)
    try:
        eng.device_upload(d_in, x)
        eng.device_upload(d_out, np.full((B + 2, w), SENTINEL, dtype=U))
        each_dev(eng, op, None, B, d_in, params, d_out + w * 8)
        # a second call straight behind the first one, on the same stream, rewrites the context's tables behind the first kernel
        each_dev(eng, op, None, B, d_in, params, d_out + w * 8)
        block = np.empty((B + 2, w), dtype=U)
        eng.device_download(None, block, d_out)
        back = np.empty_like(x)
        eng.device_download(None, back, d_in)
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)
    assert np.all(block[0] == SENTINEL) and np.all(block[B + 1] == SENTINEL), (shape, op)
    assert G.same_words(block[1:B + 1], by_batch) and G.same_words(back, x), (shape, op)
    by_group = each(groups(shape), op, x, params)                                  # items 0 .. 4 on member 0, 5 .. 8 on member 1
    assert G.same_words(by_group, by_batch), (shape, op)


def refused(eng, op, x, params, status, *texts, out=None):
    with pytest.raises(SpfError) as e:
        each(eng, op, x, params, out)
    assert e.value.status == status, (op, params, str(e.value))
    for t in texts:
        assert str(t) in str(e.value), (op, t, str(e.value))


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_refusals_carry_status_and_numbers_and_touch_nothing(rigs, shape):
    c, eng = rigs(shape)
    N, log_n = c.P.N, KC.log2n(c.P)
    x = items(c)
    for op, good, bad, status, texts in (
            ("se", 0, N, INVALID, ("parameter 4 of 9", N, "index")),
            ("ks", A, 16, INVALID, ("parameter 4 of 9", "slot 16 >= SPF_GLWE_KSK_SLOTS = 16")),
            ("ks", A, EMPTY, NO_KEY, ("parameter 4 of 9", f"slot {EMPTY}")),
            ("au", 1, 0, INVALID, ("parameter 4 of 9", f"round 0 outside 1 .. log2 N = {log_n}")),
            ("au", 1, log_n + 1, INVALID, ("parameter 4 of 9", f"round {log_n + 1} outside 1 .. log2 N = {log_n}"))):
        params = [good] * B
        params[4] = bad
        out = np.full((B, out_words(c, op)), SENTINEL, dtype=U)
        refused(eng, op, x, params, status, *texts, out=out)
        assert np.all(out == SENTINEL), (shape, op, bad)
    # MulXN amounts are taken mod 2N: none is refused
    big = each(eng, "mx", x[:2], [2 * N + 3, (1 << 64) - 1])
    assert G.same_words(big[0], oracle_row(shape, "mx", 3, 0)) and G.same_words(big[1], oracle_row(shape, "mx", ((1 << 64) - 1) % (2 * N), 1))
    # B = 0 is SPF_OK
    for op in ("se", "mx", "ks", "au"):
        assert each(eng, op, np.zeros((0, c.P.k + 1, N), dtype=U), []).shape[0] == 0
    # no automorphism key: SPF_ERR_NO_KEY
    bare = spf_amd.Engine(G.engine_params(c.P))
    try:
        out = np.full((B, out_words(c, "au")), SENTINEL, dtype=U)
        refused(bare, "au", x, [1] * B, NO_KEY, "automorphism key", out=out)
        assert np.all(out == SENTINEL)
    finally:
        bare.close()


@pytest.mark.parametrize("shape", [TUNED, SMALL])
def test_any_overlap_of_output_and_input_is_refused(rigs, shape):
    """on device pointers, where a caller can alias: out == in exactly, and the output one row into the input"""
    c, eng = rigs(shape)
    N, lib = c.P.N, eng._lib
    gw = (c.P.k + 1) * N
    x = items(c)
    d = eng.device_alloc(2 * x.nbytes)
    try:
        eng.device_upload(d, np.concatenate([x.reshape(-1), x.reshape(-1)]))
        for name, fn, good in (("se", lib.spf_sample_extract_l1_each_devptr, 0), ("mx", lib.spf_glwe_mul_xn_each_devptr, 1),
                               ("ks", lib.spf_glwe_keyswitch_each_devptr, A), ("au", lib.spf_glwe_automorphism_each_devptr, 1)):
            p = np.full(B, good, dtype=U)
            for off in (0, gw * 8, (B - 1) * gw * 8):
                st = fn(eng._h, None, B, d, p.ctypes.data_as(C.c_void_p), d + off)
                assert st == INVALID and b"overlap" in lib.spf_last_error(eng._h), (shape, name, off)
        back = np.empty(2 * x.size, dtype=U)
        eng.device_download(None, back, d)
        assert G.same_words(back[:x.size], x) and G.same_words(back[x.size:], x)
    finally:
        eng.device_free(d)


@pytest.mark.parametrize("shape", [TUNED, SMALL])
@pytest.mark.parametrize("op", ["se", "mx"])
def test_more_items_than_grid_rows_is_still_one_strided_launch(rigs, shape, op):
    """SampleExtract and MulXN put the items on grid.y, 32768 rows at most, and stride beyond: B = 32768 + 3 walks the stride once
    more for three items.  Rows on both sides of the seam, the first and the last one against the single-parameter entry point
    and the oracle; every row of a parameter against the single-parameter call over the whole batch."""
    c, eng = rigs(shape)
    N, big = c.P.N, 32768 + 3
    x = np.ascontiguousarray(np.tile(c.x, (big // KC.ITEMS + 1, 1, 1))[:big])
    three = [N - 1, 1, 0] if op == "se" else [N + 77, 2 * N - 1, 0]
    params = np.array([three[i % 3] for i in range(big)], dtype=U)
    got = each(eng, op, x, params)
    for i in (0, 1, 32766, 32767, 32768, 32769, big - 1):
        assert G.same_words(got[i], oracle_row(shape, op, int(params[i]), i % KC.ITEMS)), (shape, op, i)
    for p in three:
        at = np.nonzero(params == U(p))[0]
        assert G.same_words(got[at], single(eng, op, x[at], p)), (shape, op, p)
