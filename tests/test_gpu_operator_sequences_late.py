"""The second ring of the operators' call-sequence fuzz (tests/fuzz_operators_late.py) on the real library: the tour over every
ordered pair of kinds with a late one in it -- cluster, plane_triplets, plane_refit, farthest, orient -- in chunks, random seeds
that draw from all the kinds, and the seeds that open with an order aimed at one sharing: gl_pose / gl_idx with 12 and 4 doubles a
hypothesis, gl_src under matched rows and rows of a cloud, counter words 2 and 3 behind a double's bits and a preset, cand_keep /
ol_cnt between the radius filter and cluster, the k-NN buffers and a slot's freshness under orient, the late entries behind a run.
Every move against its own file's reference (tests/test_operator_sequences_late_host.py shows that the driver finds what is
planted).  GPU only."""
import pytest

import fuzz_operators_late as fl

pytestmark = pytest.mark.gpu

CHUNK = 36
TOUR = fl.late_tour()
SEEDS = list(range(16))


def _run(moves, seed):
    try:
        bad, log, kernels, step = fl.run_on_library(moves, seed)
    except Exception as e:  # noqa: BLE001
        # an error of the library itself, not a mismatch: nothing more is started on a device that may have faulted
        import traceback
        traceback.print_exc()
        pytest.exit(f"late operator sequence {seed}: {type(e).__name__}: {e}", returncode=3)
    print(f"{len(moves)} moves, kernels {sorted(kernels)}")
    assert bad == [] and step is None, "\n".join(log[-12:] + [f"move {step}:"] + bad)
    return kernels, log


@pytest.mark.parametrize("part", range((len(TOUR) - 1 + CHUNK - 1) // CHUNK))
def test_late_tour_of_every_pair_with_a_late_kind(part):
    """One chunk of the tour (with one move of overlap: the pair across the cut) on a fresh context."""
    _run(TOUR[part * CHUNK:(part + 1) * CHUNK + 1], part)


@pytest.mark.parametrize("seed", SEEDS)
def test_random_late_operator_sequence(seed):
    """34 moves, half of them late kinds; seeds 0 .. 5 modulo 8 begin with a scripted opening."""
    _run(fl.late_random_moves(seed), seed)
