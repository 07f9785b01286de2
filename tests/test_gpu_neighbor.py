"""Device neighbour list (e3gnn_nlist_*, csrc/neighbor.hip) vs the host list
and the oracle's brute force: identical edges, order and integer shifts (bit
for bit), edge vectors within f32 rounding.  Needs an MI355X: ``pytest -m gpu``.

The cell-list cases at the end take their geometries from tests/_cells.py;
tests/test_cells_host.py checks on the CPU that the host list equals the brute
force on them.  oracle/neighbor.py is right only for positions wrapped into
the cell, so ``brute=True`` gets wrapped copies and unwrapped positions are
compared with the host list."""
import numpy as np
import pytest
import torch

import _cells as C
from sevennet_finetuning_amd.neighbor import neighbor_list
from sevennet_finetuning_amd.structures import si_diamond

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dnl():
    from sevennet_finetuning_amd.neighbor import DeviceNeighborList
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return DeviceNeighborList('cuda:0')


def run(dnl, pos, cell, rc=5.0, pbc=(True, True, True)):
    c, n, s, v = dnl(pos, cell, rc, pbc)
    return (np.stack([c.cpu().numpy(), n.cpu().numpy()]).astype(np.int64),
            s.cpu().numpy().astype(np.float64), v.cpu().numpy())


def host_vec(pos, cell, ei, sh):
    if cell is None:
        return (pos[ei[1]] - pos[ei[0]]).astype(np.float32)
    return ((pos[ei[1]] + sh @ cell) - pos[ei[0]]).astype(np.float32)


def check(dnl, pos, cell, rc=5.0, pbc=(True, True, True), brute=False):
    ei, sh, vec = run(dnl, pos, cell, rc, pbc)
    if brute:
        from oracle.neighbor import neighbor_list as ref
        ej, sj = ref(pos, cell, rc)
    else:
        ej, sj = neighbor_list(pos, cell, rc, pbc)
    assert np.array_equal(ei, ej)
    assert np.array_equal(sh, sj)
    if ei.shape[1]:
        assert np.abs(vec - host_vec(pos, cell, ei, sh)).max() <= 1e-5
    return ei, sh


@pytest.mark.parametrize('cells', [(1, 1, 1), (2, 2, 1), (3, 3, 3), (4, 3, 2)])
def test_si_boxes_vs_bruteforce(dnl, cells):
    pos, cell = si_diamond(cells, sigma=0.05)
    check(dnl, pos, cell, brute=True)


def test_triclinic_hfo2(dnl):
    d = np.load('tests/golden/hfo2_resdat.npz')
    check(dnl, d['pos'], d['cell'], brute=True)


def test_small_primitive_cell_many_images(dnl):
    """FCC primitive Si cell (2 atoms, heights < rc): every image within rc."""
    a = 5.43
    cell = 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.float64)
    pos = np.array([[0, 0, 0], [0.25 * a, 0.25 * a, 0.25 * a]], dtype=np.float64)
    ei, _ = check(dnl, pos, cell, rc=6.0, brute=True)
    assert ei.shape[1] == 92  # 2 atoms x 46 neighbours within 6 A


def test_unwrapped_positions(dnl):
    """Atoms outside the cell (MD-style unwrapped coordinates): the shifts
    absorb the offsets, edges unchanged in geometry."""
    pos, cell = si_diamond((3, 3, 3), sigma=0.05)
    rng = np.random.default_rng(7)
    off = rng.integers(-3, 4, size=(len(pos), 3)).astype(np.float64) @ cell
    check(dnl, pos + off, cell)


def test_cluster_no_pbc(dnl):
    rng = np.random.default_rng(3)
    pos = rng.uniform(-6, 6, size=(300, 3))
    keep = [0]
    for i in range(1, len(pos)):
        if np.min(np.linalg.norm(pos[keep] - pos[i], axis=1)) > 1.6:
            keep.append(i)
    pos = pos[keep]
    ei, sh = check(dnl, pos, None, pbc=(False, False, False))
    assert not sh.any()
    # brute force over pairs
    d = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    ii, jj = np.nonzero((d < 5.0) & ~np.eye(len(pos), dtype=bool))
    assert np.array_equal(ei, np.stack([ii, jj]))


def test_isolated_and_empty(dnl):
    ei, _, _ = run(dnl, np.zeros((1, 3)), np.eye(3) * 20.0)
    assert ei.shape == (2, 0)
    ei, _, _ = run(dnl, np.zeros((0, 3)), np.eye(3) * 20.0)
    assert ei.shape == (2, 0)


def test_mixed_pbc_is_refused(dnl):
    from sevennet_finetuning_amd._lib import E3GNNError
    pos, cell = si_diamond((2, 2, 2), sigma=0.0)
    with pytest.raises(E3GNNError):
        dnl(pos, cell, 5.0, (True, True, False))


def test_bench_box_properties(dnl):
    """97,336-atom bench box: host list equality, 28 neighbours each, the
    (i, j, S) <-> (j, i, -S) symmetry, CSR order."""
    pos, cell = si_diamond((23, 23, 23), sigma=0.05)
    ei, sh = check(dnl, pos, cell)
    assert ei.shape[1] == 28 * len(pos)
    assert np.all(np.diff(ei[0]) >= 0)
    key = lambda i, j, s: ((i * len(pos) + j) * 64 + (s[:, 0] + 2) * 16 + (s[:, 1] + 2) * 4
                           + (s[:, 2] + 2))
    s = sh.astype(np.int64)
    assert np.array_equal(np.sort(key(ei[0], ei[1], s)), np.sort(key(ei[1], ei[0], -s)))


def test_energy_forces_from_device_list(dnl):
    """The device list feeds e3gnn_energy_forces directly: same energy and
    forces as with the host list."""
    from sevennet_finetuning_amd.model import E3GNNModel
    model = E3GNNModel(device='cuda:0')
    pos, cell = si_diamond((4, 4, 4), sigma=0.05)
    types = torch.full((len(pos),), model.chemical_symbols.index('Si'), dtype=torch.int32,
                       device='cuda:0')
    c, n, _, v = dnl(pos, cell, model.cutoff)
    a = model.energy_forces(types, c, n, v)
    ei, sh = neighbor_list(pos, cell, model.cutoff)
    vec = torch.tensor(host_vec(pos, cell, ei, sh), device='cuda:0')
    b = model.energy_forces(types, torch.tensor(ei[0], device='cuda:0'),
                            torch.tensor(ei[1], device='cuda:0'), vec)
    assert abs(float(a['energy']) - float(b['energy'])) <= 1e-6 * abs(float(b['energy']))
    assert (a['forces'] - b['forces']).abs().max().item() <= 1e-5


# ------------------------------------------------------------ cell-list cases
def test_sheared_cell_vs_bruteforce(dnl):
    """Heights 7.8 / 9.8 / 10.3 A against lengths 10.1 / 12.1 / 11.4 A."""
    pos, cell, _ = C.sheared_hfo2()
    check(dnl, pos, cell, brute=True)


@pytest.mark.parametrize('rc', [5.0, 6.0])
def test_unreduced_lattice_vs_bruteforce(dnl, rc):
    """Heights 2.7 / 7.3 / 10.3 A against lengths 10.1 / 24.3 / 16.8 A: two
    heights below the cutoff, R = (2, 1, 1) and (3, 1, 1) bins of stencil."""
    pos, cell, _ = C.relabelled_hfo2(wrap=True)
    ei, _ = check(dnl, pos, cell, rc=rc, brute=True)
    if rc == 5.0:
        assert ei.shape[1] == 4302


def test_unreduced_lattice_unwrapped(dnl):
    """The atoms of the original cell in the unreduced lattice: the shifts
    absorb fractional coordinates from -1.1 to 3.1 and reach |S| = 5."""
    pos, cell, _ = C.relabelled_hfo2(wrap=False)
    ei, sh = check(dnl, pos, cell)
    assert ei.shape[1] == 4302 and np.abs(sh).max() == 5


def test_bins_of_more_than_64_atoms(dnl):
    """700 atoms in 2 x 2 x 2 bins (~87 each: the second trip of the 64-lane
    loop over a bin), degrees 281..349 (sort tiles of 512)."""
    pos, cell, _ = C.dense_box()
    ei, _ = check(dnl, pos, cell)
    deg = np.bincount(ei[0], minlength=len(pos))
    assert ei.shape[1] == 221406 and deg.max() == 349


def test_few_atoms_in_a_large_cell(dnl):
    """Three atoms in a 60 A cube: 12^3 bins halved down to 3 x 3 x 6 (at most
    4 n + 64); the only edges are 0 <-> 1 across the x boundary."""
    pos, cell, _ = C.sparse_box()
    ei, sh = check(dnl, pos, cell)
    assert np.array_equal(ei, [[0, 1], [1, 0]])
    assert np.array_equal(sh, [[-1, 0, 0], [1, 0, 0]])
    check(dnl, pos, cell, brute=True)


def test_many_bins_on_one_axis(dnl):
    """HfO2 tiled (1, 1, 4): 8 bins along c, 1 and 2 along a and b."""
    pos, cell, _ = C.tiled_hfo2()
    ei, _ = check(dnl, pos, cell, brute=True)
    assert ei.shape[1] == 4 * 4302


@pytest.mark.parametrize('N', [64, 65, 66, 128, 129, 257, 513])
def test_complete_graph_degrees_at_the_sort_padding(dnl, N):
    """Every centre has degree N - 1 = 63, 64, 65, 127, 128, 256, 512: the
    bitonic sort's padding below, at and above a power of two, and the cap
    itself accepted.  The list is the full off-diagonal pair list in (i, j) order."""
    pos, _, _ = C.ball(N)
    ei, sh = check(dnl, pos, None, pbc=(False, False, False))
    ii, jj = np.nonzero(~np.eye(N, dtype=bool))
    assert np.array_equal(ei, np.stack([ii, jj]))
    assert not sh.any()


def test_degree_513_is_refused(dnl):
    """One neighbour past the cap: a handled refusal from the single-structure
    build, and the handle stays usable."""
    from sevennet_finetuning_amd._lib import E3GNNError
    pos, _, _ = C.ball(514)
    with pytest.raises(E3GNNError, match='512'):
        dnl(pos, None, 5.0, (False, False, False))
    pos, cell, _ = C.sparse_box()
    check(dnl, pos, cell)


# ------------------------------------------- refusals the device reports, three forms
CELL6 = np.eye(3) * 6.0
PAIR = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
FORMS = ('single', 'rank', 'batch')


def build_form(dnl, form, pos):
    """(ei, sh) of (pos, CELL6) at cutoff 5 from the single build, the rank build
    (world 1: local rows are the atom ids) or the batch build, where the structure
    stands second, behind the healthy PAIR."""
    if form == 'single':
        c, n, s, _ = dnl(pos, CELL6, 5.0)
    elif form == 'rank':
        d = dnl.rank_graph(pos, CELL6, 5.0, np.zeros(len(pos), dtype=np.int32), 0, 1)
        c, n, s = d['center'], d['nbr'], d['shift']
    else:
        c, n, s, _, ap, ep = dnl.batch([PAIR, pos], [CELL6, CELL6], 5.0)
        b, e = int(ep[1]), int(ep[2])
        c, n, s = c[b:e] - int(ap[1]), n[b:e] - int(ap[1]), s[b:e]
    return (np.stack([c.cpu().numpy(), n.cpu().numpy()]).astype(np.int64),
            s.cpu().numpy().astype(np.float64))


def refused(dnl, form, pos, what):
    """The build (or its fetch) raises `what`, the batch naming structure 1;
    afterwards the same handle builds the healthy cell as the host list has it."""
    from sevennet_finetuning_amd._lib import E3GNNError
    with pytest.raises(E3GNNError, match='structure 1.*' + what if form == 'batch' else what):
        build_form(dnl, form, pos)
    ei, sh = build_form(dnl, form, PAIR)
    ej, sj = neighbor_list(PAIR, CELL6, 5.0)
    assert ej.shape[1] == 4
    assert np.array_equal(ei, ej) and np.array_equal(sh, sj)


@pytest.mark.parametrize('form', FORMS)
def test_shift_beyond_1024_cells_is_refused(dnl, form):
    """The second atom 2000 cells along a: every edge has |Sx| of 2000 or 2001,
    more than the sort key holds.  The fill pass flags it and still sorts and
    writes keys it can index with."""
    far = PAIR + np.array([[0.0, 0.0, 0.0], [2000 * 6.0, 0.0, 0.0]])
    ei, sh = neighbor_list(far, CELL6, 5.0)
    assert ei.shape[1] == 4 and set(np.abs(sh[:, 0]).tolist()) == {2000, 2001}
    refused(dnl, form, far, '1024')


@pytest.mark.parametrize('form', FORMS)
def test_non_finite_position_is_refused(dnl, form):
    bad = PAIR.copy()
    bad[1, 1] = np.nan
    refused(dnl, form, bad, 'non-finite')
