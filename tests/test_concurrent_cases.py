"""The job table of the concurrency tests (tests/concurrent_cases.py) and its checker, shown without a GPU.

The table: every job has an answer for every worker; no two workers of a job share one (a worker that reads another's scratch,
workspace or output then shows); an output is never what its pre-fill already holds; and for the two-launch reductions the answer
of worker k differs from the three things a crossed finalize step can produce — the fold of another worker's partials, of too
few of its own, of too few of another's.

The checker: the ways a concurrent call can go wrong, as edits of the expected outputs — two workers' outputs swapped, an output
left at its pre-fill, one tile of another worker's output pasted in, a record with one field from another worker — are each
reported, for every job."""
import numpy as np
import pytest

import concurrent_cases as K

JOBS = K.JOBS
IDS = [j.name for j in JOBS]
WORKERS = range(K.WORKERS)
TILE = 256      # bytes pasted by the tile fault: one workgroup's lanes of the narrowest cell


def test_the_table_names_every_family():
    for name in ("ec_compare", "ec_compare_scalar", "ec_select", "ec_masked_select", "ec_cast", "ec_cast_scaled", "ec_window(copy)",
                 "ec_window(nearest)", "ec_window_put", "ec_window_resample(average)", "ec_window_resample(bilinear)", "ec_focal(sum)",
                 "ec_focal(min)", "ec_focal_convolve", "ec_focal_rank(median)", "ec_focal_majority", "ec_composite", "ec_composite_rank",
                 "ec_reclass", "ec_stats_device", "ec_stats_device(one workgroup)", "ec_stats_compute", "ec_zonal_stats_device",
                 "ec_zonal_stats_compute", "ec_zonal_broadcast", "ec_distance(caller's workspace)", "ec_distance(library's workspace)",
                 "ec_regions(caller's workspace)", "ec_regions(library's workspace)", "ec_min_max_keys", "ec_mask_counts_device",
                 "ec_expr_min_max_keys", "ec_first_difference", "ec_min_max", "ec_mask_counts"):
        assert name in K.BY_NAME, name


def test_cell_types_rotate_over_every_width():
    """among the workers of the families that take a cell type: a 1-byte, a 2-byte and an 8-byte cell"""
    for job in JOBS:
        types = {job.inputs(k)["t"] for k in WORKERS if "t" in job.inputs(k)}
        if len(types) > 1:
            assert {1, 2, 8} <= {K.size_of(t) for t in types}, job.name


@pytest.mark.parametrize("job", JOBS, ids=IDS)
def test_every_worker_has_its_own_answer(job):
    want = [job.expected(k) for k in WORKERS]
    for k in WORKERS:
        assert want[k] and all(len(v) > 0 for v in want[k].values()), (job.name, k)
        assert set(job.host) <= set(want[k]) and set(job.records) <= set(want[k]), job.name
        for name, v in want[k].items():
            assert v != bytes([K.fill_byte(k)]) * len(v), (job.name, k, name, "the answer is the pre-fill")
        for j in range(k):
            assert want[j] != want[k], (job.name, j, k)
    sizes = [tuple(len(v) for v in w.values()) for w in want]
    if max(sizes[0]) > 4096:     # rasters: no two workers share an output size
        assert len(set(sizes)) == len(sizes), (job.name, sizes)


def test_make_is_deterministic():
    for job in JOBS[:6]:
        a, b = job.make(3), job.make(3)
        for name, v in a.items():
            assert np.array_equal(v, b[name]) if isinstance(v, np.ndarray) else v == b[name], (job.name, name)


REDUCTIONS = [j for j in JOBS if j.reduction]


def test_the_reductions_are_the_two_launch_ones():
    assert [j.name for j in REDUCTIONS] == ["ec_stats_device", "ec_min_max_keys", "ec_mask_counts_device", "ec_expr_min_max_keys", "ec_first_difference"]


@pytest.mark.parametrize("job", REDUCTIONS, ids=[j.name for j in REDUCTIONS])
def test_a_crossed_finalize_is_wrong_for_certain(job):
    """Worker k's answer against the answer over every other worker's cells, over its own first g tiles for every g below its
    grid, and over every other worker's first g tiles.  The grids are 2, 3, 4 and 5 workgroups."""
    tile_of, prefix = job.reduction
    whole, parts = {}, {}
    for j in WORKERS:
        inp = job.inputs(j)
        t, n = tile_of(inp), inp["x"].size
        grid = -(-n // t)
        assert grid == j % 4 + 2 and n == (grid - 1) * t + 2 * j + 3, (job.name, j, n, t)
        whole[j] = job.expected(j)
        for g in range(1, grid):
            parts[j, g] = job.want(prefix(inp, g * t))
    for k in WORKERS:
        for j in WORKERS:
            if j != k:
                assert whole[k] != whole[j], (job.name, k, "equals worker", j)
        for (j, g), w in parts.items():
            assert whole[k] != w, (job.name, k, "equals the first", g, "tiles of worker", j)


def test_the_extremes_sit_in_the_last_tile_and_belong_to_one_worker():
    seen = set()
    for job in (K.BY_NAME["ec_stats_device"], K.BY_NAME["ec_min_max_keys"]):
        for k in WORKERS:
            inp = job.inputs(k)
            a, m, t = inp["x"], inp["mask"], K.tile(inp["t"])
            last = (a.size - 1) // t * t
            vis = a if m is None else a[m != 0]
            assert a[-1] == vis.min() and a[-2] == vis.max() and (a[:last] > a[-1]).all() and (a[:last] < a[-2]).all(), (job.name, k)
            if m is not None:
                hidden = a[last:-2]
                assert (m[last:-2] == 0).all() and hidden.min() < a[-1] and hidden.max() > a[-2], (job.name, k)
            for v in (int(a[-1]), int(a[-2])):
                assert (job.name, inp["t"], v) not in seen
                seen.add((job.name, inp["t"], v))


# ---------------------------------------------------------------- the checker against the ways a concurrent call goes wrong
def other(k):
    return (k + 3) % K.WORKERS


@pytest.mark.parametrize("job", JOBS, ids=IDS)
def test_the_checker_passes_the_right_answer_and_reports_every_fault(job):
    for k in WORKERS:
        want, theirs, fill = job.expected(k), job.expected(other(k)), K.fill_byte(k)
        assert K.check(want, dict(want), fill) == [], (job.name, k)

        # two workers' outputs swapped
        assert K.check(want, dict(theirs), fill), (job.name, k, "swapped")

        # an output left at its pre-fill, one output at a time
        for name, v in want.items():
            got = dict(want)
            got[name] = bytes([fill]) * len(v)
            report = K.check(want, got, fill)
            assert len(report) == 1 and "pre-fill" in report[0], (job.name, k, name, report)
            got.pop(name)
            assert K.check(want, got, fill), (job.name, k, name, "missing")

        # one tile of another worker's output pasted in, at the first place where the two differ
        pasted = 0
        for name, v in want.items():
            at = K.first_difference(v, theirs[name])
            if at is None:
                continue
            at -= at % TILE
            end = min(at + TILE, len(v), len(theirs[name]))
            got = dict(want)
            got[name] = v[:at] + theirs[name][at:end] + v[end:]
            assert len(got[name]) == len(v) and K.check(want, got, fill), (job.name, k, name, "tile")
            pasted += 1
        assert pasted, (job.name, k, "no output differs from worker", other(k), "within their common length")

        # a record with one field from another worker
        for name in job.records:
            v, w = want[name], theirs[name]
            swapped = 0
            for at in range(0, min(len(v), len(w)) - 7, 8):
                if v[at:at + 8] != w[at:at + 8]:
                    got = dict(want)
                    got[name] = v[:at] + w[at:at + 8] + v[at + 8:]
                    assert K.check(want, got, fill), (job.name, k, name, at)
                    swapped += 1
            assert swapped, (job.name, k, name, "no field differs")
