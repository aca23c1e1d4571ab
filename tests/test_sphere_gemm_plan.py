"""CPU: the one split plan behind every sphere integral (``csrc/sphere_gemm.h``), restated here and held against
the four ``*_work_floats`` queries of the built library, which are pure host arithmetic over the shape.

The plan decides the order in which an output element's terms are added, so the renders, the prefiltered maps, their
gradients and the needlet coefficients change bits when it changes; the scratch sizes are where it shows without a GPU.  The
sweep reaches every clip of the plan: more than 512 row groups (one split), fewer chunks than wanted splits, the cap of 64
splits, a ragged last chunk, chunks per split that do not divide the chunks, and the refused shapes, which give 0."""
import itertools

import pytest

ROWS_WG, CHUNK, SLOTS, MAX_SPLIT = 128, 64, 512, 64


def split_plan(rows, k, seen=None):
    """(nchunks, per, splits, rowgroups) of a reduction over k entries for `rows` rows; nothing else enters."""
    nchunks, rowgroups = -(-k // CHUNK), -(-rows // ROWS_WG)
    want = max(1, min(SLOTS // rowgroups, MAX_SPLIT, nchunks))
    per = -(-nchunks // want)
    splits = -(-nchunks // per)
    if seen is not None:
        seen |= {name for name, hit in (("one split: more than 512 row groups", rowgroups > SLOTS),
                                        ("fewer chunks than wanted", nchunks < min(SLOTS // rowgroups, MAX_SPLIT)),
                                        ("the cap of 64", SLOTS // rowgroups > MAX_SPLIT <= nchunks),
                                        ("ragged last chunk", k % CHUNK != 0),
                                        ("per does not divide", nchunks % per != 0),
                                        ("fewer splits than wanted", splits < want)) if hit}
    return nchunks, per, splits, rowgroups


ALL_CLIPS = {"one split: more than 512 row groups", "fewer chunks than wanted", "the cap of 64", "ragged last chunk",
             "per does not divide", "fewer splits than wanted"}


def inside_count(S):
    """Pixels of the S x S image inside the sphere's disc: X^2 + Y^2 < S^2 on the odd lattice."""
    return sum((2 * j + 1 - S) ** 2 + (S - 1 - 2 * i) ** 2 < S * S for i in range(S) for j in range(S))


def needlet_rows(jmax):
    return 4 ** (jmax + 2) - 3


@pytest.fixture(scope="module")
def L():
    from emlight_amd import _lib
    return _lib.lib()


def test_the_restated_plan_on_literal_cases():
    assert split_plan(208, 32768) == (512, 8, 64, 2)              # S = 16 against 128 x 256: the cap
    assert split_plan(3228, 32768) == (512, 27, 19, 26)           # S = 64: floor(512 / 26) = 19 wanted, 27 does not divide 512
    assert split_plan(16384, 576) == (9, 3, 3, 128)               # 4 wanted, 3 chunks each: the fourth split would be empty
    assert split_plan(70000, 32768) == (512, 512, 1, 547)         # more row groups than slots
    assert split_plan(60, 288) == (5, 1, 5, 1)                    # 5 chunks, the last of 32
    assert split_plan(8192, 2 * 128 * 128) == (512, 64, 8, 64)    # Ho = 64 against 128 x 256


def test_sphere_render_work_floats_follow_the_plan(L):
    seen = set()
    counts = {S: inside_count(S) for S in (2, 8, 9, 16, 33, 64, 150, 300)}
    for (S, P), H, B in itertools.product(counts.items(), (1, 4, 12, 16, 45, 128), (1, 2, 11)):
        T = 2 * H * H
        splits = split_plan(P, T, seen)[2]
        assert L.eml_sphere_render_work_floats(B, H, 2 * H, S) == 4 * T + 8 * P + splits * 2 * P * 3 * B, (B, H, S)
    assert seen == ALL_CLIPS
    # the split does not see the batch
    P = counts[16]
    w1, w7 = (L.eml_sphere_render_work_floats(B, 128, 256, 16) for B in (1, 7))
    assert (w7 - 4 * 32768 - 8 * P) == 7 * (w1 - 4 * 32768 - 8 * P)
    for B, H, W, S in ((0, 16, 32, 8), (1, 16, 33, 8), (1, 16, 16, 8), (1, 0, 0, 8), (1, 4097, 8194, 8), (1, 16, 32, 1),
                       (1, 16, 32, 1025), (4097, 16, 32, 8), (-1, 16, 32, 8)):
        assert L.eml_sphere_render_work_floats(B, H, W, S) == 0, (B, H, W, S)


def test_env_prefilter_work_floats_follow_the_plan_both_ways(L):
    fwd, bwd = set(), set()
    for H, Ho, B, lobes in itertools.product((1, 4, 12, 16, 45, 128, 200), (1, 4, 7, 8, 64, 100, 182), (1, 3, 33), (1, 4)):
        T, D = 2 * H * H, 2 * Ho * Ho
        assert L.eml_env_prefilter_work_floats(B, H, 2 * H, Ho, lobes) == \
            4 * T + 4 * D + split_plan(D, T, fwd)[2] * 2 * D * 3 * B, (B, H, Ho)
        assert L.eml_env_prefilter_bwd_work_floats(B, H, 2 * H, Ho, lobes) == \
            4 * T + 4 * D + split_plan(T, D, bwd)[2] * T * 3 * B, (B, H, Ho)
    assert fwd == ALL_CLIPS and bwd == ALL_CLIPS
    for f in (L.eml_env_prefilter_work_floats, L.eml_env_prefilter_bwd_work_floats):
        for B, H, W, Ho, lobes in ((0, 16, 32, 8, 1), (1, 16, 33, 8, 1), (1, 0, 0, 8, 1), (1, 4097, 8194, 8, 1), (1, 16, 32, 0, 1),
                                   (1, 16, 32, 1025, 1), (1, 16, 32, 8, 0), (1, 16, 32, 8, 9), (4097, 16, 32, 8, 1)):
            assert f(B, H, W, Ho, lobes) == 0, (B, H, W, Ho, lobes)


def test_needlet_work_floats_follow_the_plan(L):
    seen = set()
    for jmax, P, B in itertools.product(range(5), (1, 63, 64, 288, 700, 3072, 5000, 12288, 32768, 1 << 24), (1, 11, 33)):
        K = needlet_rows(jmax)
        assert L.eml_needlet_work_floats(P, jmax, B) == split_plan(K, P, seen)[2] * K * 3 * B, (P, jmax, B)
    assert seen == ALL_CLIPS - {"one split: more than 512 row groups"}    # 4093 rows are 32 row groups at the most
    for P, jmax, B in ((64, 2, 0), (64, -1, 1), (64, 5, 1), (0, 2, 1), ((1 << 24) + 1, 2, 1), (64, 2, 65536)):
        assert L.eml_needlet_work_floats(P, jmax, B) == 0, (P, jmax, B)
