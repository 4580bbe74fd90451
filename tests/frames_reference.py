"""The frames render's restatement (include/cudabrot_amd.h, "Frames render") -- test infrastructure only.

By the section's Consequence, the frames render of (matrices, ...) IS the stack of the projected (or Julia) renders with
each matrix, each on the same generators: plot_reference.draw(..., projection=P_f) over f, every frame on a fresh copy of
the generator states.  The counters are frame 0's with `increments` summed over the frames.  No C of its own."""

import numpy as np

import plot_reference as plot


def draw(lib, matrices, w, h, max_iter, min_iter, n_threads, launches, *, states=None, seed=1337, first_subsequence=0,
         **kw):
    """-> (u64 hist [F, h, w], counters dict).  matrices: [F, 8] or F matrices [2][4].  kw: plot_reference.draw's degree,
    ship, formula, c, box, omp_threads.  Given `states` are advanced in place, once."""
    from oracle import binding

    frames = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 8)
    start = binding.init_states(seed, first_subsequence, n_threads) if states is None else states
    planes, counters, after = [], None, None
    for p in frames:
        own = start.copy()  # every frame draws the same samples
        hist, cnt = plot.draw(lib, w, h, max_iter, min_iter, n_threads, launches, projection=p, states=own, **kw)
        planes.append(hist)
        if counters is None:
            counters, after = dict(cnt), own
        else:
            assert {k: v for k, v in cnt.items() if k != "increments"} == {k: v for k, v in counters.items()
                                                                          if k != "increments"}
            assert own.tobytes() == after.tobytes()
            counters["increments"] += cnt["increments"]
    if states is not None:
        states[...] = after
    return np.stack(planes), counters
