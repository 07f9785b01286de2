"""Dataset inference on the HIP path: many structures per device build and
evaluation -- the loop of the reference's ``sevenn_inference``
(sevenn/scripts/inference.py:185-291: ``set_is_batch_data(True)``, graphs from
``AtomsToGraphCollater``, one model call per batch) and its error summary
(``get_error_recorder``, :77-92).

``predict_many`` groups consecutive structures up to an atom budget; each group
is one ``DeviceNeighborList.batch`` build and one
``E3GNNModel.energy_forces_batch`` evaluation, whose per-structure sums run in a
fixed order on the device (bitwise reproducible).  Structures periodic in one or
two dimensions only (slabs, wires) take the calculator's single-structure path.
"""
import numpy as np
import torch

KBAR = 1602.1766208   # eV/A^3 -> kbar (error_recorder.py ERROR_TYPES['Stress'])


def group_batches(sizes, max_atoms_per_batch):
    """Consecutive groups of structure indices: a group is closed when the next
    structure would take it past ``max_atoms_per_batch`` atoms, so the input
    order is kept and a structure larger than the budget gets a group of its
    own.  ``sizes``: atoms per structure."""
    if max_atoms_per_batch < 1:
        raise ValueError('max_atoms_per_batch must be at least 1')
    groups, cur, tot = [], [], 0
    for k, n in enumerate(sizes):
        n = int(n)
        if cur and tot + n > max_atoms_per_batch:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(k)
        tot += n
    if cur:
        groups.append(cur)
    return groups


def _calculator(model_or_calculator):
    from .sevennet_calculator import SevenNetCalculator
    if isinstance(model_or_calculator, SevenNetCalculator):
        return model_or_calculator
    return SevenNetCalculator(model_or_calculator)


def _predict_group(calc, atoms_group):
    """One device build and one evaluation for structures that are each fully
    periodic or fully isolated."""
    from .neighbor import DeviceNeighborList
    if calc._nlist is None:
        calc._nlist = DeviceNeighborList(calc.device)
    model = calc.model
    pbcs = [bool(np.all(a.get_pbc())) for a in atoms_group]
    cells = [np.array(a.get_cell(), dtype=np.float64) if p else None
             for a, p in zip(atoms_group, pbcs)]
    center, nbr, _, vec, atom_ptr, _ = calc._nlist.batch(
        [a.get_positions() for a in atoms_group], cells, calc.cutoff, [(p,) * 3 for p in pbcs])
    types = torch.as_tensor(np.concatenate([calc._types(a) for a in atoms_group]),
                            dtype=torch.int32, device=calc.device)
    res = model.energy_forces_batch(types, center, nbr, vec, atom_ptr, want_virial=any(pbcs))
    energy = res['energy'].cpu().numpy()
    energies = res['atomic_energy'].cpu().numpy()
    forces = res['forces'].cpu().numpy()
    virial = res['virial'].cpu().numpy() if any(pbcs) else None
    out, a0 = [], 0
    for k, atoms in enumerate(atoms_group):
        a1 = a0 + len(atoms)
        r = {'energy': float(energy[k]), 'energies': energies[a0:a1].copy(),
             'forces': forces[a0:a1].copy()}
        if pbcs[k]:
            # the calculator's convention: -sigma in ASE's Voigt order xx yy zz yz xz xy
            sigma = virial[k] / abs(np.linalg.det(cells[k]))
            r['stress'] = -sigma[[0, 1, 2, 4, 5, 3]]
        out.append(r)
        a0 = a1
    return out


def predict_many(model_or_calculator, atoms_list, max_atoms_per_batch=4096):
    """Energies, forces and stresses of many structures.

    ``model_or_calculator``: a ``SevenNetCalculator``, or a loaded model / model
    name as its constructor takes.  ``atoms_list``: ``ase.Atoms`` (or
    ``structures.Atoms``) objects.  Consecutive structures are grouped up to
    ``max_atoms_per_batch`` atoms (``group_batches``): one device graph build and
    one evaluation per group.  Returns, in input order, one dict per structure:
    ``energy`` (eV), ``energies`` [n], ``forces`` [n, 3] and, for periodic cells,
    ``stress`` [6] with the calculator's sign and Voigt order.  A structure
    periodic in only one or two dimensions is evaluated by
    ``SevenNetCalculator.calculate`` (host graph)."""
    calc = _calculator(model_or_calculator)
    if not hasattr(calc.model, 'energy_forces_batch'):
        from ._lib import E3GNNError
        raise E3GNNError('predict_many needs the native engine (load_model(engine="native")): '
                         'the torch engine has no batched evaluation')
    atoms_list = list(atoms_list)
    out = [None] * len(atoms_list)
    batched = []
    for k, atoms in enumerate(atoms_list):
        pbc = np.asarray(atoms.get_pbc(), dtype=bool).reshape(-1)
        if len(atoms) > 0 and (pbc.all() or not pbc.any()):
            batched.append(k)
        else:
            calc.calculate(atoms)
            out[k] = {key: calc.results[key] for key in ('energy', 'energies', 'forces', 'stress')
                      if key in calc.results}
    for group in group_batches([len(atoms_list[k]) for k in batched], max_atoms_per_batch):
        idx = [batched[g] for g in group]
        for k, r in zip(idx, _predict_group(calc, [atoms_list[k] for k in idx])):
            out[k] = r
    return out


def errors(predictions, references):
    """The six numbers of the reference's inference summary (get_error_recorder,
    sevenn/scripts/inference.py:77-92; error_recorder.py RMSError / MAError):

    * ``energy_rmse`` / ``energy_mae``: energy per atom (eV/atom) over structures;
    * ``force_rmse``: root of the mean over atoms of |dF|^2 (the reference's
      vector form, vdim 3); ``force_mae``: mean over force components (eV/A);
    * ``stress_rmse``: root of the mean over structures of the summed squares of
      the six components; ``stress_mae``: mean over components -- in kbar
      (x 1602.1766208), over the structures that have a stress on both sides
      (nan when none has).

    ``predictions`` / ``references``: sequences of dicts with ``energy``,
    ``forces`` and optionally ``stress`` (``predict_many``'s output)."""
    if len(predictions) != len(references):
        raise ValueError('predictions and references must have the same length')
    de, df, ds = [], [], []
    for p, r in zip(predictions, references):
        fp = np.asarray(p['forces'], dtype=np.float64).reshape(-1, 3)
        fr = np.asarray(r['forces'], dtype=np.float64).reshape(-1, 3)
        if fp.shape != fr.shape:
            raise ValueError('a prediction and its reference differ in atom count')
        de.append((float(p['energy']) - float(r['energy'])) / max(len(fp), 1))
        df.append(fp - fr)
        if p.get('stress') is not None and r.get('stress') is not None:
            ds.append((np.asarray(p['stress'], dtype=np.float64).reshape(6)
                       - np.asarray(r['stress'], dtype=np.float64).reshape(6)) * KBAR)
    de = np.array(de, dtype=np.float64)
    df = np.concatenate(df) if df else np.zeros((0, 3))
    ds = np.array(ds, dtype=np.float64).reshape(-1, 6)
    nan = float('nan')
    return {
        'energy_rmse': float(np.sqrt(np.mean(de ** 2))) if len(de) else nan,
        'force_rmse': float(np.sqrt(np.mean((df ** 2).sum(1)))) if len(df) else nan,
        'stress_rmse': float(np.sqrt(np.mean((ds ** 2).sum(1)))) if len(ds) else nan,
        'energy_mae': float(np.mean(np.abs(de))) if len(de) else nan,
        'force_mae': float(np.mean(np.abs(df))) if len(df) else nan,
        'stress_mae': float(np.mean(np.abs(ds))) if len(ds) else nan,
    }
