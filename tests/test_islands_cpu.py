"""The preconditions of test_hip_list_edges.py, proved with the CPU oracle alone: every frame that file hands to the library
has exactly the list lengths (and, for the shell islands, the candidate counts) its tests are named after, so that none of
their assertions can hold vacuously.  Nothing here touches the device."""
import numpy as np
import pytest

import islands
from islands import A, A_SIZES, B, B_SIZES, SHELL, SHELL_SIZES, SKIN, SPECIES


def _lengths(frame, rc):
    """By the linked-cell builder of the oracle, which the GPU tests use as well (the all-pairs one takes a second per call on
    these frames; _check_islands holds the two against each other once per geometry)."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc, isl = frame
    ptr, j, off = orc.neighbors_cells(pos, cell, pbc, rc)
    return np.diff(ptr), (ptr, j, off)


_checked = set()


def _check_islands(frame, rc, sizes):
    """Every atom of island k has exactly sizes[k] - 1 neighbours, all of them of its own island; no pair of the frame lies
    within 1e-6 A of the cut-off or of the candidate cut-off (where the oracle and the device could round apart)."""
    from oracle import oracle as orc
    numbers, pos, cell, pbc, isl = frame
    nn, (ptr, j, off) = _lengths(frame, rc)
    assert len(numbers) == sum(sizes) and np.array_equal(np.bincount(isl), sizes)
    for k, n in enumerate(sizes):
        assert set(nn[isl == k].tolist()) == {n - 1}, (k, n, np.unique(nn[isl == k]))
    assert set(nn.tolist()) == {n - 1 for n in sizes}
    i = np.repeat(np.arange(len(numbers)), nn)
    assert np.array_equal(isl[i], isl[j])
    assert np.all(pos >= 0) and np.all(pos < cell[0, 0]) and (off != 0).any()    # wrapped, and some lists cross a cell face
    for cut in (rc, rc + SKIN):
        assert orc.neighbors_cells(pos, cell, pbc, cut - 1e-6)[0][-1] == orc.neighbors_cells(pos, cell, pbc, cut + 1e-6)[0][-1]
    if pos.tobytes() not in _checked:   # (the positions do not depend on the species table)
        _checked.add(pos.tobytes())
        for x, y in zip(orc.neighbors(pos, cell, pbc, rc), (ptr, j, off)):
            assert np.array_equal(x, y)
    return nn


def _check_species(frame, species):
    """Every species of the table occurs in every island — in every list-length class, whatever slot count is compiled."""
    numbers, _, _, _, isl = frame
    for k in range(isl.max() + 1):
        assert set(numbers[isl == k].tolist()) == set(species), k


@pytest.mark.parametrize("nspec", sorted({s for _, _, s in islands.FORMS}))
def test_frame_a_has_the_nine_lengths(nspec):
    frame = islands.frame_a(SPECIES[:nspec])
    nn = _check_islands(frame, A["rc"], A_SIZES)
    assert sorted(set(nn.tolist())) == [47, 48, 49, 63, 64, 65, 127, 128, 129]
    assert len(nn) == 729 and frame[2][0, 0] == 66.0
    _check_species(frame, SPECIES[:nspec])
    # the candidates (rc + skin) are the neighbours: the sort and hit-mask edges are crossed at the same atoms
    assert np.array_equal(_lengths(frame, A["rc"] + SKIN)[0], nn)


@pytest.mark.parametrize("sizes", islands.ROWS16_SIZES)
@pytest.mark.parametrize("nspec", [1, 2, 3])
def test_rows16_frames_end_at_63_64_65(sizes, nspec):
    frame = islands.frame_a(SPECIES[:nspec], sizes)
    nn = _check_islands(frame, A["rc"], sizes)
    assert nn.max() == {3: 63, 4: 64, 5: 65}[len(sizes)]
    _check_species(frame, SPECIES[:nspec])


@pytest.mark.parametrize("nspec", sorted({s for _, _, s in islands.MD_FORMS}))
def test_md_frame_has_48_64_128(nspec):
    frame = islands.frame_a(SPECIES[:nspec], islands.MD_SIZES)
    nn = _check_islands(frame, A["rc"], islands.MD_SIZES)
    assert sorted(set(nn.tolist())) == [48, 64, 128]
    _check_species(frame, SPECIES[:nspec])


def test_frame_b_straddles_the_sort_limit():
    frame = islands.frame_b(SPECIES[:3])
    nn = _check_islands(frame, B["rc"], B_SIZES)
    assert sorted(set(nn.tolist())) == [255, 256, 257] and len(nn) == 771 and frame[2][0, 0] == 52.0
    _check_species(frame, SPECIES[:3])
    assert np.array_equal(_lengths(frame, B["rc"] + SKIN)[0], nn)


def test_shell_islands_have_exact_candidates_and_fewer_hits():
    """At every step of the walk of the reuse test: candidate counts {63, 64, 65, 127, 128, 129} by island; every island
    whose count is on or above a tile edge (64, 65, 128, 129) has an atom with fewer hits than that edge — so the hit mask
    has a word that is not full and the list is shorter than the candidate row; no atom further than 0.02 A from where the
    candidates were built (a tenth of what forces a rebuild), except atom 0 at the step that carries it through the cell."""
    numbers, pos, cell, pbc, isl = frame = islands.shell_frame(SPECIES[:3])
    rc = SHELL["rc"]
    _check_species(frame, SPECIES[:3])
    frames = islands.shell_walk(pos, cell)
    assert len(frames) == islands.SHELL_STEPS and np.array_equal(frames[0], pos)
    for step, p in enumerate(frames):
        base = pos.copy()
        if step >= islands.SHELL_REBUILD:
            base[0] += cell[0]
        assert np.linalg.norm(p - base, axis=1).max() <= 0.02 * (1 + 1e-12)
        assert step == 0 or np.linalg.norm(p - base, axis=1).max() > 0.015
        ncand, (ptr, j, off) = _lengths((numbers, p, cell, pbc, isl), rc + SKIN)
        i = np.repeat(np.arange(len(numbers)), ncand)
        assert np.array_equal(isl[i], isl[j])
        nn, _ = _lengths((numbers, p, cell, pbc, isl), rc)
        for k, n in enumerate(SHELL_SIZES):
            assert set(ncand[isl == k].tolist()) == {n - 1}, (step, k)
            assert nn[isl == k].min() < n - 1 and len(set(nn[isl == k].tolist())) > 1, (step, k)
            if n - 1 >= 127:
                assert nn[isl == k].min() > 64, (step, k)            # ... and still two words of hits
    assert sorted(set(ncand.tolist())) == [63, 64, 65, 127, 128, 129]
    assert (off != 0).any()


@pytest.mark.parametrize("which,lmax,nmax,nspec", [("a", 3, 3, 3), ("a", 3, 3, 12), ("a", 4, 4, 2), ("b", 3, 3, 3), ("shell", 3, 3, 3)])
def test_island_forces_sum_to_zero_in_the_oracle(which, lmax, nmax, nspec):
    """Islands do not interact, so the oracle's forces sum to zero island by island (to 1e-12 of the largest force): what
    the GPU tests ask of the library at 1e-10 is a property of the model, not of the frame as a whole."""
    from oracle import oracle as orc
    species = SPECIES[:nspec]
    make, kw = {"a": (islands.frame_a, A), "b": (islands.frame_b, B), "shell": (islands.shell_frame, SHELL)}[which]
    numbers, pos, cell, pbc, isl = make(species)
    rc, eta, m = kw["rc"], 4.0, 24
    X = islands.inducing(numbers, pos, cell, pbc, rc, m, seed=2)
    ind_z, ind_ptr, bz, br = islands.inducing_arrays(X)
    assert set(ind_z.tolist()) == set(species)
    Pm, nnm = orc.inducing_descriptors(lmax, nmax, rc, species, ind_z, ind_ptr, bz, br)
    M = orc.kernel_matrix(ind_z, nnm, Pm, ind_z, nnm, Pm, eta)
    assert np.linalg.cond(M) < 1e4   # (tens to hundreds for lmax = 3, above a thousand for (4, 4) with two species)
    mu = np.random.default_rng(9).normal(size=m)
    nl = orc.neighbors(pos, cell, pbc, rc)
    ref = orc.frame(lmax, nmax, rc, eta, species, numbers, pos, cell, nl, ind_z, nnm, Pm, mu, want_p=False)
    fmax = np.abs(ref["forces"]).max()
    assert fmax > 0
    for k in range(isl.max() + 1):
        assert np.abs(ref["forces"][isl == k].sum(0)).max() <= 1e-12 * fmax, k
