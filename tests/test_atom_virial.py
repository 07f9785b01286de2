"""Per-atom virial, the parts that need no GPU: the C ABI entry and its
binding, the torch partition helper, and the decomposed driver's extra
reverse exchange on the CPU segment engine (gloo, two ranks).

The quantity is the edge-gradient partition of the virial (_atom_virial.py,
DESIGN.md "Per-atom virial"); the device kernel is checked in
test_gpu_atom_virial.py.
"""
import re
import socket
import subprocess

import numpy as np
import torch
import torch.multiprocessing as mp

from _atom_virial import edge_terms, partition
from _systems import load_manifest_symbols, system
from sevennet_finetuning_amd import _lib


def test_header_declares_and_library_exports_atom_virial():
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r'int\s+e3gnn_atom_virial\s*\(\s*e3gnn_ctx\s*\*\s*c\s*,\s*float\s*\*\s*atom_virial6\s*,'
                     r'\s*void\s*\*\s*stream\s*\)\s*;', text)
    assert 'e3gnn_atom_virial' in _lib.header_symbols()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True,
                         text=True).stdout
    assert any(line.split()[-1] == 'e3gnn_atom_virial' and ' T ' in line for line in out.splitlines())


def test_lib_binds_atom_virial_and_refuses_null_arguments():
    import ctypes
    res, args = _lib.SIGNATURES['e3gnn_atom_virial']
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 3
    lib = _lib.load()
    assert lib.e3gnn_atom_virial.argtypes == args
    assert lib.e3gnn_abi_version() == 1          # an addition: the version stays
    assert lib.e3gnn_atom_virial(None, None, None) == 1   # E3GNN_ERR_ARG, no device touched
    assert b'null context' in lib.e3gnn_last_error()


def test_torch_partition_matches_a_direct_loop():
    """model.atom_virial_partition against the definition written as a loop
    over edges, on a random graph with edges from an atom to its own image
    (centre == neighbour: both halves on one atom) and an atom without edges."""
    from sevennet_finetuning_amd.model import atom_virial_partition
    rng = np.random.default_rng(5)
    n, E = 7, 40
    center = np.sort(rng.integers(0, n - 1, E))     # atom n - 1 has no edge
    nbr = rng.integers(0, n - 1, E)
    nbr[::5] = center[::5]                          # self-image edges
    vec, grad = rng.normal(size=(E, 3)), rng.normal(size=(E, 3))
    want = np.zeros((n, 6))
    for e in range(E):
        r, g = vec[e], grad[e]
        v = -np.array([r[0] * g[0], r[1] * g[1], r[2] * g[2], 0.5 * (r[0] * g[1] + r[1] * g[0]),
                       0.5 * (r[1] * g[2] + r[2] * g[1]), 0.5 * (r[0] * g[2] + r[2] * g[0])])
        want[center[e]] += 0.5 * v
        want[nbr[e]] += 0.5 * v
    got = atom_virial_partition(n, torch.tensor(center), torch.tensor(nbr), torch.tensor(vec),
                                torch.tensor(grad)).numpy()
    assert got.shape == (n, 6) and got.dtype == np.float64
    assert np.abs(got - want).max() < 1e-14
    assert np.all(got[n - 1] == 0) and (nbr == center).sum() >= 8
    # rows sum to the total virial; the numpy helper of the GPU tests agrees
    assert np.abs(got.sum(0) - edge_terms(vec, grad)[0].sum(0)).max() < 1e-13
    assert np.abs(partition(n, center, nbr, vec, grad)[0] - want).max() < 1e-14


def test_decomposed_atom_virial_matches_the_serial_partition(tmp_path):
    """Two gloo ranks on the fp64 CPU segment engine: the per-atom virial
    gathered by owner after the extra reverse exchange equals the partition of
    the single-process oracle's edge gradient to 1e-10; the option costs
    exactly one exchange and leaves energy and forces bit for bit."""
    from _atom_virial_workers import worker
    from oracle.neighbor import neighbor_list
    from oracle.sevennet_ref import SevenNet0Ref
    name = 'si_rng0_2x2x2'
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    out = str(tmp_path / 'w2.npz')
    mp.spawn(worker, args=(2, port, name, 'cpu', out), nprocs=2, join=True)
    got = np.load(out)
    pos, cell, types = system(name, load_manifest_symbols())
    ref = SevenNet0Ref(dtype=torch.float64)
    ei, sh = neighbor_list(pos, cell, ref.cutoff)
    o = ref.energy(torch.tensor(pos).requires_grad_(True), torch.tensor(types), torch.tensor(ei), torch.tensor(sh),
                   torch.tensor(cell), False)
    g, = torch.autograd.grad(o['energy'], o['edge_vec'])
    want, _, _ = partition(len(pos), ei[0], ei[1], o['edge_vec'].detach().numpy(), g.numpy())
    assert got['rows'][2] > 0 and got['rows'][0] == got['rows'][1]   # ghosts exist; owned rows returned
    assert np.abs(want).max() > 0.1
    assert np.abs(got['atomic_virial'] - want).max() < 1e-10
    assert np.abs(got['atomic_virial'].sum(0) - got['virial']).max() < 1e-10
    assert got['exchanges'][1] == got['exchanges'][0] + 1
    assert got['same'][0] and not got['default_has_key'][0]
