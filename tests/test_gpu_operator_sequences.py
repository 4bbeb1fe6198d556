"""The call-sequence fuzz of the operators (tests/fuzz_operators.py) on the real library: the tour over every ordered pair of
operator kinds in chunks, random seeds, and the seeds that open with an order aimed at one sharing -- degrees and then inlier counts
through gl_idx, the chain's three on alternating roads, a mask count before a preset word before the sweeps' words, a run's slots
against the stand-alone search's, an upload between two users of the normal cache.  Every move against its own file's reference
(tests/test_operator_sequences_host.py shows that the driver finds what is planted).  GPU only."""
import pytest

import fuzz_operators as fo

pytestmark = pytest.mark.gpu

CHUNK = 36
TOUR = fo.tour()
SEEDS = list(range(32))


def _run(moves, seed):
    try:
        bad, log, kernels, step = fo.run_on_library(moves, seed)
    except Exception as e:  # noqa: BLE001
        # an error of the library itself, not a mismatch: nothing more is started on a device that may have faulted
        import traceback
        traceback.print_exc()
        pytest.exit(f"operator sequence {seed}: {type(e).__name__}: {e}", returncode=3)
    print(f"{len(moves)} moves, kernels {sorted(kernels)}")
    assert bad == [] and step is None, "\n".join(log[-12:] + [f"move {step}:"] + bad)
    return kernels, log


@pytest.mark.parametrize("part", range((len(TOUR) - 1 + CHUNK - 1) // CHUNK))
def test_tour_of_every_ordered_pair(part):
    """One chunk of the tour (with one move of overlap: the pair across the cut) on a fresh context."""
    _run(TOUR[part * CHUNK:(part + 1) * CHUNK + 1], part)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_operator_sequence(seed):
    """34 moves; seeds 0 .. 4 modulo 8 begin with a scripted opening."""
    moves = fo.random_moves(seed)
    kernels, log = _run(moves, seed)
    if seed % 8 == 3:
        # the opening's run goes through the filtered search (1 000 queries, the threshold forced to 512)
        assert "k_grid_nn16f" in kernels, (kernels, log)
