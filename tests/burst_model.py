"""numpy statement of include/fosphor_amd_burst.h, twice.

bursts()        rules 1 - 5 as the header words them: on cells, gap closing, runs numbered row-major, links between runs of rows up to
                max_gap_rows + 1 apart whose column intervals intersect, a plain union-find, records per component.
flood_bursts()  shares no code with it: the gap-closed bitmap is made cell by cell, and components are a pixel flood fill in which
                horizontally adjacent cells, and cells (j, i) and (j + k, i) with 1 <= k <= max_gap_rows + 1, are neighbours; the
                records come from each component's list of pixels.  It knows nothing of runs, so it gives no n_runs.

Written from the definitions, not from the kernels; tests/test_burst_cpu.py compares the two with each other and the library's host
function with them, tests/test_gpu_burst.py compares the device with bursts().  ys is always [rows][n] by source index j (0 = newest)
and window column; thr a scalar or [n]; columns are reported with first_bin added."""
import numpy as np

F32 = np.float32
BURST_DTYPE = np.dtype([("newest", "<i4"), ("oldest", "<i4"), ("first_col", "<i4"), ("last_col", "<i4"), ("n_cells", "<i4"),
                        ("peak_row", "<i4"), ("peak_col", "<i4"), ("peak_y", "<f4"), ("energy_y", "<f4"), ("flags", "<u4")])
RESULT_NAMES = ("n_runs", "n_components", "n_found", "n_written", "overflow")
CFG_DTYPE = np.dtype([("first_bin", "<i4"), ("n_cols", "<i4"), ("rows", "<i4"), ("threshold_y", "<f4"), ("max_gap_cols", "<i4"),
                      ("max_gap_rows", "<i4"), ("min_rows", "<i4"), ("min_cols", "<i4"), ("max_runs", "<i4")])
RESULT_DTYPE = np.dtype([(k, "<i4") for k in RESULT_NAMES])
ON, CUT, FIRST_COL, LAST_COL = 1, 2, 4, 8


def on_cells(ys, thr):
    """rule 1: plain float32 y > thr[i]; a NaN on either side is False"""
    ys = np.asarray(ys, F32)
    t = np.broadcast_to(np.asarray(thr, F32), ys.shape[-1:])
    with np.errstate(invalid="ignore"):
        return ys > t[None, :]


def energy_y(terms_y):
    """0.5 * log10 of the fp64 sum of the finite 10^(2 y)"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        t = np.power(10.0, 2.0 * np.asarray(terms_y, np.float64))
        return F32(0.5 * np.log10(np.where(np.isfinite(t), t, 0.0).sum()))


def flags_of(newest, oldest, first, last, rows, n):
    return (ON if newest == 0 else 0) | (CUT if oldest == rows - 1 else 0) | (FIRST_COL if first == 0 else 0) | \
           (LAST_COL if last == n - 1 else 0)


def row_runs(on_row, max_gap_cols):
    """rule 2 for one row: (firsts, lasts) of its runs.  A gap is closed when it is no longer than max_gap_cols and has an on cell
    on both sides, which a gap at an edge has not."""
    idx = np.flatnonzero(on_row)
    if idx.size == 0:
        return idx, idx
    cut = np.flatnonzero(np.diff(idx) - 1 > max_gap_cols)		# the gaps that stay open
    return idx[np.concatenate(([0], cut + 1))], idx[np.concatenate((cut, [idx.size - 1]))]


def finish(res_runs, comps, rows, n, first_bin, min_rows, min_cols, max_bursts):
    """rule 4 on the components' records (a BURST_DTYPE array in ascending root order, columns relative to the window, flags not
    yet set): flags, filters, n_found, the first max_bursts"""
    comps = comps.copy()
    comps["flags"] = np.where(comps["newest"] == 0, ON, 0) | np.where(comps["oldest"] == rows - 1, CUT, 0) | \
        np.where(comps["first_col"] == 0, FIRST_COL, 0) | np.where(comps["last_col"] == n - 1, LAST_COL, 0)
    kept = comps[(comps["oldest"] - comps["newest"] + 1 >= min_rows) & (comps["last_col"] - comps["first_col"] + 1 >= min_cols)]
    out = kept[:max_bursts].copy()
    for name in ("first_col", "last_col", "peak_col"):
        out[name] += first_bin
    res = dict(n_runs=res_runs, n_components=len(comps), n_found=len(kept), n_written=int(out.size), overflow=0)
    return res, out


def bursts(ys, thr, first_bin=0, max_gap_cols=0, max_gap_rows=0, min_rows=1, min_cols=1, max_bursts=65536, max_runs=1 << 20):
    """(result dict, records) by rules 1 - 5"""
    ys = np.asarray(ys, F32)
    rows, n = ys.shape
    on = on_cells(ys, thr)
    firsts, lasts, row_off = [], [], [0]
    for j in range(rows):
        f, l = row_runs(on[j], max_gap_cols)
        firsts.append(f)
        lasts.append(l)
        row_off.append(row_off[-1] + f.size)
    n_runs = row_off[-1]
    if n_runs > max_runs:						# rule 5
        return dict(n_runs=n_runs, n_components=0, n_found=0, n_written=0, overflow=1), np.zeros(0, BURST_DTYPE)
    if n_runs == 0:
        return dict(n_runs=0, n_components=0, n_found=0, n_written=0, overflow=0), np.zeros(0, BURST_DTYPE)
    first, last = np.concatenate(firsts), np.concatenate(lasts)
    row = np.repeat(np.arange(rows), np.diff(row_off))

    # rule 3: a plain union-find over every linked pair, the root the lowest run number
    parent = list(range(n_runs))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for k in range(1, max_gap_rows + 2):
        for j in range(rows - k):
            a0, a1, b0, b1 = row_off[j], row_off[j + 1], row_off[j + k], row_off[j + k + 1]
            if a0 == a1 or b0 == b1:
                continue
            lo = np.searchsorted(last[b0:b1], first[a0:a1], side="left")		# the first run of row j + k that ends at or after mine begins
            hi = np.searchsorted(first[b0:b1], last[a0:a1], side="right")	# one past the last that begins at or before mine ends
            for a in np.flatnonzero(hi > lo):
                for b in range(lo[a], hi[a]):
                    assert first[a0 + a] <= last[b0 + b] and first[b0 + b] <= last[a0 + a]
                    ra, rb = find(a0 + a), find(b0 + b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(r) for r in range(n_runs)])
    roots, comp_of = np.unique(root, return_inverse=True)		# ascending roots
    assert np.array_equal(roots, np.flatnonzero(root == np.arange(n_runs)))

    # the cells of every run, row-major, with the component they belong to
    length = last - first + 1
    cell_run = np.repeat(np.arange(n_runs), length)
    cell_col = np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length) + first[cell_run]
    cell_row = row[cell_run]
    cell_y = ys[cell_row, cell_col]
    cell_comp = comp_of[cell_run]
    nc = roots.size
    newest = np.full(nc, rows); np.minimum.at(newest, comp_of, row)
    oldest = np.full(nc, -1); np.maximum.at(oldest, comp_of, row)
    fcol = np.full(nc, n); np.minimum.at(fcol, comp_of, first)
    lcol = np.full(nc, -1); np.maximum.at(lcol, comp_of, last)
    n_cells = np.bincount(cell_comp, minlength=nc)
    with np.errstate(over="ignore", invalid="ignore"):
        term = np.power(10.0, 2.0 * cell_y.astype(np.float64))
    esum = np.bincount(cell_comp, weights=np.where(np.isfinite(term), term, 0.0), minlength=nc)
    valid = ~np.isnan(cell_y)
    peak = np.full(nc, -np.inf, F32); np.maximum.at(peak, cell_comp[valid], cell_y[valid] + F32(0))		# -0 counts as +0
    with np.errstate(invalid="ignore"):
        at_peak = np.flatnonzero(valid & (cell_y == peak[cell_comp]))			# row-major: the first of a component wins the tie
    which, where = np.unique(cell_comp[at_peak], return_index=True)
    assert np.array_equal(which, np.arange(nc)), "a component without a peak"
    where = at_peak[where]
    with np.errstate(divide="ignore"):
        e_y = (0.5 * np.log10(esum)).astype(F32)
    comps = np.zeros(nc, BURST_DTYPE)
    for name, a in (("newest", newest), ("oldest", oldest), ("first_col", fcol), ("last_col", lcol), ("n_cells", n_cells),
                    ("peak_row", cell_row[where]), ("peak_col", cell_col[where]), ("peak_y", peak), ("energy_y", e_y)):
        comps[name] = a
    return finish(n_runs, comps, rows, n, first_bin, min_rows, min_cols, max_bursts)


def closed_bitmap(ys, thr, max_gap_cols):
    """the on-or-closed cells, cell by cell: a not-on cell is closed when the maximal not-on stretch it lies in is no longer than
    max_gap_cols and ends on an on cell at either side"""
    ys = np.asarray(ys, F32)
    rows, n = ys.shape
    t = np.broadcast_to(np.asarray(thr, F32), (n,))
    out = np.zeros((rows, n), bool)
    for j in range(rows):
        on = [bool(ys[j, i] > t[i]) for i in range(n)]
        i = 0
        while i < n:
            if on[i]:
                out[j, i] = True
                i += 1
                continue
            k = i
            while k < n and not on[k]:
                k += 1
            if i > 0 and k < n and k - i <= max_gap_cols:
                out[j, i:k] = True
            i = k
    return out


def flood_bursts(ys, thr, first_bin=0, max_gap_cols=0, max_gap_rows=0, min_rows=1, min_cols=1, max_bursts=65536):
    """(result dict with n_runs None, records) by pixel flood fill"""
    ys = np.asarray(ys, F32)
    rows, n = ys.shape
    bitmap = closed_bitmap(ys, thr, max_gap_cols)
    seen = np.zeros((rows, n), bool)
    comps = []
    for j0 in range(rows):						# row-major seeds: components come in ascending root order
        for i0 in range(n):
            if not bitmap[j0, i0] or seen[j0, i0]:
                continue
            seen[j0, i0] = True
            stack, pixels = [(j0, i0)], []
            while stack:
                j, i = stack.pop()
                pixels.append((j, i))
                near = [(j, i - 1), (j, i + 1)]
                near += [(j + k, i) for k in range(1, max_gap_rows + 2)] + [(j - k, i) for k in range(1, max_gap_rows + 2)]
                for jj, ii in near:
                    if 0 <= jj < rows and 0 <= ii < n and bitmap[jj, ii] and not seen[jj, ii]:
                        seen[jj, ii] = True
                        stack.append((jj, ii))
            pixels.sort()
            js, cols = [q[0] for q in pixels], [q[1] for q in pixels]
            best = None
            for j, i in pixels:					# ascending (j, column): a strict > keeps the first of equals
                y = ys[j, i]
                if not np.isnan(y) and (best is None or y > ys[best]):
                    best = (j, i)
            comps.append(dict(newest=min(js), oldest=max(js), first_col=min(cols), last_col=max(cols), n_cells=len(pixels),
                              peak_row=best[0], peak_col=best[1], peak_y=ys[best], energy_y=energy_y([ys[q] for q in pixels])))
    arr = np.zeros(len(comps), BURST_DTYPE)
    for k, c in enumerate(comps):
        for name, v in c.items():
            arr[name][k] = v
    return finish(None, arr, rows, n, first_bin, min_rows, min_cols, max_bursts)


def energy_error(got, want):
    """worst |got - want| over energy_y, equal infinities counting as 0; inf where one side alone is not finite"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.where(g == w, 0.0, np.abs(g - w))
    err = np.where(np.isnan(err), np.inf, err)
    return float(err.max()) if err.size else 0.0


def assert_bursts_equal(got, want, tol, tag=""):
    """integers, peak and flags with equality (peak_y as a float: -0 is +0), energy_y within tol"""
    assert len(got) == len(want), (tag, "records", len(got), len(want))
    for k in ("newest", "oldest", "first_col", "last_col", "n_cells", "peak_row", "peak_col", "peak_y", "flags"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (tag, k, "burst", int(bad[0]), got[k][bad[0]], want[k][bad[0]], got[bad[0]], want[bad[0]])
    err = energy_error(got["energy_y"], want["energy_y"])
    assert err <= tol, (tag, "energy_y", err)
    return err


def assert_result_equal(got, want, tag=""):
    for k in RESULT_NAMES:
        if want[k] is not None:
            assert int(got[k]) == int(want[k]), (tag, k, int(got[k]), int(want[k]))
