"""Device loader, the parts that need no GPU: the padding contract
(_collate_ref.py) against train.collate, the shape buckets as pure logic, the
refusals of the C ABI's dataset / collate entries, and a padded batch trained
against the unpadded one on the CPU double of the convolution."""
import ctypes

import numpy as np
import pytest
import torch

from _collate_ref import padded_batch, same_bits
from _conv_cpu import CpuConvBackend
from _systems import load_manifest_symbols
from sevennet_finetuning_amd import _keys as KEY
from sevennet_finetuning_amd import _lib, train
from sevennet_finetuning_amd.structures import diamond_primitive, mixed_symbols
from sevennet_finetuning_amd.train_data import DeviceDataset, DeviceLoader, plan_shapes

SYMS = load_manifest_symbols()
RC = 5.0
ERR_ARG = 1


def structure(cells, seed):
    pos, cell = diamond_primitive(cells, sigma=0.3, seed=seed)
    types = np.array([SYMS.index(s) for s in mixed_symbols(len(pos), seed=seed + 1)])
    rng = np.random.default_rng(1000 + seed)
    return (pos, cell, types, -4.0 * len(pos) + rng.normal(0, 0.5),
            rng.normal(0, 0.3, (len(pos), 3)), rng.normal(0, 2e-3, 6))


def graph(cells, seed):
    pos, cell, types, e, f, s = structure(cells, seed)
    return train.labeled_graph(pos, cell, types, RC, energy=e, force=f, stress=s)


# ------------------------------------------------------------- 1. the contract
def test_contract_statement_against_collate():
    gs = [graph((2, 2, 1), 1), graph((2, 2, 2), 2), graph((3, 2, 2), 3)]
    assert [int(g[KEY.NUM_ATOMS]) for g in gs] == [8, 16, 24]
    ref = train.collate(gs, dtype=torch.float32)
    A, E = 48, int(ref[KEY.EDGE_IDX].shape[1])
    real_deg = int(np.bincount(ref[KEY.EDGE_IDX][0].numpy()).max())
    slots, atom_cap, edge_cap = 5, A + 6, E + 13          # 2 dummy slots, 6 dummy atoms
    r_pad = np.float32(RC)
    b = padded_batch(gs, slots, atom_cap, edge_cap, r_pad, with_shift=True)
    # the real prefix is collate's output bit for bit
    for k, rows in ((KEY.NODE_FEATURE, A), (KEY.FORCE, A), (KEY.BATCH, A), (KEY.EDGE_VEC, E),
                    (KEY.CELL_SHIFT, E), (KEY.NUM_ATOMS, 3), (KEY.CELL_VOLUME, 3),
                    (KEY.ENERGY, 3), (KEY.STRESS, 3)):
        assert b[k].shape[0] == {A: atom_cap, E: edge_cap, 3: slots}[rows], k
        assert same_bits(b[k][:rows], ref[k].numpy()), k
    assert same_bits(b[KEY.EDGE_IDX][:, :E], ref[KEY.EDGE_IDX].numpy())
    assert b[KEY.EDGE_IDX].shape == (2, edge_cap)
    # the padded part
    assert b[KEY.NUM_ATOMS][3:].tolist() == [1, 5] and b[KEY.NUM_ATOMS].sum() == atom_cap
    assert (b[KEY.NUM_ATOMS][3:] >= 1).all()
    assert b[KEY.BATCH][A:].tolist() == [3, 4, 4, 4, 4, 4]
    assert (b[KEY.NODE_FEATURE][A:] == 0).all()
    assert np.isnan(b[KEY.FORCE][A:]).all() and np.isnan(b[KEY.ENERGY][3:]).all()
    assert np.isnan(b[KEY.STRESS][3:]).all()
    assert (b[KEY.CELL_VOLUME][3:] == 1.0).all()
    pc, pn = b[KEY.EDGE_IDX][0, E:], b[KEY.EDGE_IDX][1, E:]
    assert np.array_equal(pc, pn)                                   # self edges
    assert pc.min() >= A and pc.max() < atom_cap                    # of dummy atoms only
    assert (b[KEY.EDGE_IDX][:, :E] < A).all()                       # none touches a real atom
    assert (np.diff(b[KEY.EDGE_IDX][0]) >= 0).all()                 # CSR order through the batch
    assert same_bits(b[KEY.EDGE_VEC][E:], np.tile(np.array([r_pad, 0, 0], np.float32), (13, 1)))
    assert np.linalg.norm(b[KEY.EDGE_VEC][E:].astype(np.float64), axis=1).tolist() == [float(r_pad)] * 13
    assert (b[KEY.CELL_SHIFT][E:] == 0).all()
    assert np.bincount(pc - A).tolist() == [3, 3, 3, 3, 1]          # blocks of ceil(13 / 6)
    assert np.bincount(pc - A).max() <= real_deg
    # no padded edge at all: the dummy atoms are isolated
    b0 = padded_batch(gs, 4, A + 1, E, r_pad)
    assert b0[KEY.EDGE_IDX].shape == (2, E) and b0[KEY.NUM_ATOMS].tolist() == [8, 16, 24, 1]


# ------------------------------------------------------------- 2. the buckets
class StubDataset:
    """sizes and buffers of a DeviceDataset on the host; ``collate_into``
    applies the argument rules of e3gnn_dataset_collate instead of launching"""
    device, has_shift, cutoff = torch.device('cpu'), False, RC

    def __init__(self, atoms, edges, max_degree):
        self.atoms, self.edges = np.asarray(atoms, np.int64), np.asarray(edges, np.int64)
        self.max_degree = max_degree
        self.calls = []

    def __len__(self):
        return len(self.atoms)

    def sizes(self):
        return self.atoms, self.edges

    def empty_batch(self, slots, atom_cap, edge_cap):
        return DeviceDataset.empty_batch(self, slots, atom_cap, edge_cap)

    def collate_into(self, index, slots, out):
        atom_cap, edge_cap = out[KEY.NODE_FEATURE].shape[0], out[KEY.EDGE_IDX].shape[1]
        n_real, a, e = len(index), int(self.atoms[index].sum()), int(self.edges[index].sum())
        assert 1 <= n_real <= slots - 1 <= 63
        assert a + (slots - n_real) <= atom_cap and e <= edge_cap
        dummies, pad = atom_cap - a, edge_cap - e
        assert -(-pad // dummies) <= self.max_degree
        self.calls.append(np.array(index))


def _mixed_sizes(S=37, seed=3):
    rng = np.random.default_rng(seed)
    atoms = rng.choice([8, 16, 24, 54], S)
    return atoms, atoms * 28 - rng.integers(0, 40, S)


def test_bucket_properties_over_200_epochs():
    atoms, edges = _mixed_sizes()
    ds = StubDataset(atoms, edges, max_degree=28)
    for nb in (1, 2, 3):
        ld = DeviceLoader(ds, batch_size=4, shuffle=True, seed=11, n_edge_buckets=nb)
        assert len(ld) == 10 and 1 <= len(ld.shapes) <= nb
        assert ld.edge_caps[-1] == np.sort(edges)[-4:].sum()
        assert ld.edge_caps[0] >= np.sort(edges)[:4].sum()
        sigs, orders = set(), []
        for epoch in range(200):
            ds.calls.clear()
            n_batches = 0
            for b in ld:
                n_batches += 1
                sigs.add(train.GraphedRehearsalStep._sig(b))
                assert train.edges_marked_sorted(b)
                shape = (b[KEY.NODE_FEATURE].shape[0], b[KEY.EDGE_IDX].shape[1])
                assert shape in ld.shapes and b[KEY.NUM_ATOMS].shape[0] == 5
                # the smallest capacity that holds the batch
                e = edges[ds.calls[-1]].sum()
                assert shape[1] == min(c for c in ld.edge_caps if c >= e)
            assert n_batches == 10 and len(ds.calls[-1]) == 1          # the short last batch
            seen = np.concatenate(ds.calls)
            assert sorted(seen.tolist()) == list(range(37))            # each exactly once
            assert np.array_equal(seen, np.random.default_rng(11 + epoch).permutation(37))
            orders.append(seen)
            caps = sum(ld.capacity_of(ix) for ix in ds.calls)
            assert ld.pad_fraction == (caps - edges.sum()) / edges.sum()
        assert len(sigs) <= nb
        assert len({tuple(o) for o in orders}) == 200                  # epochs differ
    # same seed, same orders; another seed, others; no shuffle: dataset order
    a = DeviceLoader(ds, 4, seed=5)
    b = DeviceLoader(ds, 4, seed=5)
    c = DeviceLoader(ds, 4, seed=6)
    for k in range(3):
        assert np.array_equal(a.order(k), b.order(k)) and not np.array_equal(a.order(k), c.order(k))
    ds.calls.clear()
    assert len(list(DeviceLoader(ds, 4, shuffle=False))) == 10
    assert np.concatenate(ds.calls).tolist() == list(range(37))
    # more buckets never pad more
    pf = []
    for nb in (1, 2, 4):
        ld = DeviceLoader(ds, 4, seed=0, n_edge_buckets=nb)
        list(ld)
        pf.append(ld.pad_fraction)
    assert pf[0] >= pf[1] >= pf[2] > 0


def test_memory_loader_restarted_mid_epoch():
    """the rehearsal loop's use: next() until StopIteration, then iter() again"""
    atoms, edges = _mixed_sizes(S=9, seed=4)
    mem_ds = StubDataset(atoms, edges, max_degree=28)
    mem = DeviceLoader(mem_ds, batch_size=4, seed=2)
    it, drawn = iter(mem), []
    for _ in range(8):                      # 3 batches per pass: restarts inside the 8 draws
        try:
            next(it)
        except StopIteration:
            it = iter(mem)
            next(it)
        drawn.append(mem_ds.calls[-1])
    want = [ix for k in range(3) for ix in mem.batch_indices(k)][:8]
    assert mem.epoch == 3 and len(drawn) == len(want)
    for got, w in zip(drawn, want):
        assert np.array_equal(got, w)
    for k in range(2):                      # the complete passes hold every structure once
        assert sorted(np.concatenate(drawn[3 * k:3 * k + 3]).tolist()) == list(range(9))


def test_plan_shapes_edge_cases():
    # one structure size: one capacity whatever the bucket count; the dummy slot's atom
    assert plan_shapes([54] * 16, [1512] * 16, 8, 2, 28) == (8 * 54 + 1, [8 * 1512])
    # the short last batch decides: 1 structure in the capacity of 8 needs
    # ceil((8 * 1512 - 1512) / 27) = 392 dummy atoms beside its 54
    assert plan_shapes([54] * 17, [1512] * 17, 8, 2, 27) == (54 + 392, [8 * 1512])
    # fewer structures than a batch
    assert plan_shapes([8, 16], [200, 400], 8, 2, 28) == (24 + 7, [600])
    with pytest.raises(ValueError, match='batch_size'):
        plan_shapes([8], [200], 64, 2, 28)
    with pytest.raises(ValueError, match='n_edge_buckets'):
        plan_shapes([8], [200], 1, 0, 28)


# ------------------------------------------------------------- 3. ABI refusals
def _i64(a):
    return (ctypes.c_int64 * len(a))(*a) if a is not None else None


def test_dataset_and_collate_argument_rules():
    """Every refusal returns E3GNN_ERR_ARG with its message, before any HIP
    call: the device pointers are fakes that are never dereferenced, and a HIP
    call would return E3GNN_ERR_HIP on a machine without a GPU."""
    lib = _lib.load()
    for name in ('e3gnn_dataset_create', 'e3gnn_dataset_free', 'e3gnn_dataset_collate'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    fake = 1 << 20
    names = [f[0] for f in _lib.DatasetArrays._fields_]

    def create(S=3, atom_ptr=(0, 8, 24, 48), edge_ptr=(0, 100, 300, 600), arrays=True, **null):
        a = _lib.DatasetArrays(**{k: (None if null.get(k, False) else fake) for k in names})
        h = lib.e3gnn_dataset_create(0, S, _i64(atom_ptr), _i64(edge_ptr),
                                     ctypes.byref(a) if arrays else None)
        return h, lib.e3gnn_last_error().decode()

    def no_dataset(**kw):
        h, msg = create(**kw)
        assert not h, msg
        return msg

    assert 'number of structures' in no_dataset(S=0)
    assert 'null atom_ptr' in no_dataset(atom_ptr=None)
    assert 'null edge_ptr' in no_dataset(edge_ptr=None)
    assert 'null arrays' in no_dataset(arrays=False)
    assert 'atom_ptr[0]' in no_dataset(atom_ptr=(1, 8, 24, 48))
    assert 'edge_ptr[0]' in no_dataset(edge_ptr=(1, 100, 300, 600))
    assert 'structure 1 is empty' in no_dataset(atom_ptr=(0, 8, 8, 48))
    assert 'edge_ptr decreases at structure 2' in no_dataset(edge_ptr=(0, 100, 300, 200))
    assert 'null atom array' in no_dataset(type=True)
    assert 'null edge array' in no_dataset(edge_vec=True)
    assert 'null per-structure array' in no_dataset(volume=True)

    h, _ = create(shift=True)          # no shifts held
    hs, _ = create()                   # shifts held
    assert h and hs
    fields = [f[0] for f in _lib.BatchArrays._fields_]
    good = dict(index=[2, 0], slots=3, atom_cap=40, edge_cap=450, max_degree=28, r_pad=5.0)

    def refused(handle=h, null=(), out=True, **change):
        a = {**good, **change}
        b = _lib.BatchArrays(**{k: (None if k in null else fake) for k in fields})
        idx = a['index']
        rc = lib.e3gnn_dataset_collate(handle, len(idx) if idx is not None else 1, _i64(idx),
                                       a['slots'], a['atom_cap'], a['edge_cap'], a['max_degree'],
                                       a['r_pad'], ctypes.byref(b) if out else None, None)
        assert rc == ERR_ARG, (rc, lib.e3gnn_last_error().decode())
        return lib.e3gnn_last_error().decode()

    assert 'null dataset handle' in refused(handle=None)
    assert 'null batch arrays' in refused(out=False)
    for k in fields:
        if k != 'pbc_shift':
            assert 'null batch buffer' in refused(null=(k,)), k
    assert 'pbc_shift' in refused(handle=hs, null=('pbc_shift',))
    assert 'null index list' in refused(index=None)
    assert 'index 3 (entry 1) outside [0, 3)' in refused(index=[0, 3])
    assert 'index -1 (entry 0) outside [0, 3)' in refused(index=[-1, 0])
    assert '3 real structures in 3 slots' in refused(index=[0, 1, 2])
    assert 'slot count must be in [2, 64]' in refused(slots=65, index=[0] * 64)
    assert 'slot count must be in [2, 64]' in refused(slots=1, index=[])
    # 24 + 8 real atoms and one dummy slot: 33 rows at least
    assert '32 real atoms plus one atom for each of the 1 dummy slots exceed the atom capacity 32' \
        in refused(atom_cap=32)
    assert 'exceed the atom capacity 33' in refused(atom_cap=33, slots=4)     # two dummy slots
    assert '400 real edges exceed the edge capacity 399' in refused(edge_cap=399)
    # 50 padded edges over 1 dummy atom, cap 28; two dummy atoms hold them
    msg = refused(atom_cap=33)
    assert '50 padded edges over 1 dummy atoms' in msg and 'above the degree cap 28' in msg
    assert 'degree cap 0' in refused(max_degree=0)
    for bad in (0.0, -5.0, float('nan'), float('inf')):
        assert 'r_pad must be finite and positive' in refused(r_pad=bad)
    assert 'capacities out of range' in refused(atom_cap=1 << 31)
    lib.e3gnn_dataset_free(h)
    lib.e3gnn_dataset_free(hs)
    lib.e3gnn_dataset_free(None)


# ------------------------------------------------- 4. padded vs unpadded step
@pytest.mark.parametrize('static', [False, True], ids=['eager-loss', 'static-loss'])
def test_padded_batch_trains_like_the_unpadded_one(static):
    """Trainable model on the CPU double, fp32: the loss and the flat parameter
    gradient of a padded batch (two real structures, a 3-atom dummy carrying 7
    padded edges) equal the unpadded batch's within 1e-5 relative (the
    project's graphed-vs-eager loss bar; 1e-5 in relative norm for the
    gradient), in the losses' eager form (NaN labels indexed out) and in the
    static form of the captured step (ref := pred).  Dummy forces are exactly
    0: at r = rc the cutoff polynomial has a double root."""
    from sevennet_finetuning_amd.nn import SevenNetTrainable
    torch.manual_seed(0)
    model = SevenNetTrainable(device='cpu', conv_backend=CpuConvBackend())
    assert model.dtype == torch.float32
    cfg = {'loss': 'huber', 'loss_param': {'delta': 0.01}, 'force_loss_weight': 1.0,
           'stress_loss_weight': 0.01, 'is_train_stress': True, 'optimizer': 'adam',
           'optim_param': {'lr': 1e-4}, 'scheduler': 'exponentiallr',
           'scheduler_param': {'gamma': 0.99}, 'device': 'cpu'}
    tr = train.Trainer(model, cfg)
    model.train(True)
    gs = [graph((2, 2, 1), 5), graph((2, 2, 1), 6)]
    plain = train.collate(gs, dtype=torch.float32)
    E = int(plain[KEY.EDGE_IDX].shape[1])
    r_pad = np.float32(model.cutoff)
    assert float(r_pad) == float(torch.tensor(model.cutoff, dtype=torch.float32))
    padded = {k: torch.from_numpy(v) for k, v in padded_batch(gs, 3, 16 + 3, E + 7, r_pad).items()}
    train.mark_edges_sorted(padded)

    def loss_and_grad(batch, static_form):
        for f, _ in tr.loss_functions:
            f.static = static_form
        tr.zero_grad()
        loss, out = tr.loss_backward(batch)
        return float(loss.detach()), model.flat_grad.detach().double().clone(), out

    l0, g0, _ = loss_and_grad(plain, False)
    l1, g1, out = loss_and_grad(padded, static)
    print(f'loss {l0:.9g} vs {l1:.9g} (rel {abs(l1 - l0) / abs(l0):.2e}), '
          f'grad rel norm {float((g1 - g0).norm() / g0.norm()):.2e}')
    assert np.isfinite(l1) and torch.isfinite(g1).all()
    assert abs(l1 - l0) <= 1e-5 * abs(l0)
    assert float((g1 - g0).norm() / g0.norm()) <= 1e-5
    assert out[KEY.PRED_TOTAL_ENERGY].shape == (3,) and out[KEY.PRED_FORCE].shape == (19, 3)
    assert torch.isfinite(out[KEY.PRED_FORCE]).all()
    assert (out[KEY.PRED_FORCE][16:] == 0).all()
    assert (out[KEY.PRED_STRESS][2] == 0).all()
