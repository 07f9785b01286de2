"""e3gnn_error_sums on the GPU against the module's torch-f64 sums
(error_recorder.error_sums_torch) on the same f32 tensors.

Bound: 1e-12 relative on every sum, counts exact.  Both sides add at most
2e4 non-negative f64 terms formed exactly from the f32 inputs (the kernel is
built without contraction), so only the order of the additions differs: below
n 2^-53 relative."""
import numpy as np
import pytest
import torch

from sevennet_finetuning_amd import _lib
from sevennet_finetuning_amd.error_recorder import KBAR, error_sums_torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NS = _lib.ERR_SUMS_PER_QUANTITY
COUNTS = [q * NS + s for q in range(_lib.ERR_QUANTITIES) for s in (_lib.ERRS_COMPONENTS, _lib.ERRS_VECTORS)]
DELTA = 0.05      # entries on both sides of it in every quantity (asserted below)


def case(nb, n, seed, all_nan=False):
    rng = np.random.default_rng(seed)
    natoms = rng.integers(1, 60, nb)
    e_ref = rng.normal(-200, 50, nb)
    f_ref = rng.normal(0, 1, (n, 3))
    s_ref = rng.normal(0, 2e-3, (nb, 6))
    # errors from far below DELTA to far above it (stress: in kbar)
    e_pred = e_ref + natoms * rng.normal(0, DELTA, nb) * rng.choice([0.1, 10], nb)
    f_pred = f_ref + rng.normal(0, DELTA, (n, 3)) * rng.choice([0.1, 10], (n, 3))
    s_pred = s_ref + rng.normal(0, DELTA / KBAR, (nb, 6)) * rng.choice([0.1, 10], (nb, 6))
    if all_nan:
        e_ref[:], f_ref[:], s_ref[:] = np.nan, np.nan, np.nan
        # predictions under dropped labels are never read into a sum
        e_pred[::2], f_pred[::3], s_pred[::2] = np.nan, np.inf, -np.inf
    elif n > 8:
        f_ref[rng.integers(0, n, max(1, n // 50)), rng.integers(0, 3, max(1, n // 50))] = np.nan
        f_pred[np.isnan(f_ref)] = np.inf
        if nb > 2:
            e_ref[1], s_ref[2, 4], s_ref[0] = np.nan, np.nan, np.nan
            e_pred[1] = np.nan
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)   # noqa: E731
    return dict(e_pred=f32(e_pred), e_ref=f32(e_ref), natoms=torch.tensor(natoms, device=DEV),
                f_pred=f32(f_pred), f_ref=f32(f_ref), s_pred=f32(s_pred), s_ref=f32(s_ref))


def kernel(c, criterion, sums, stress=True):
    nb, n = int(c['e_pred'].numel()), int(c['f_pred'].shape[0])
    p = lambda k: c[k].data_ptr()   # noqa: E731
    _lib.check(_lib.load().e3gnn_error_sums(
        criterion, DELTA, nb, n, p('e_pred'), p('e_ref'), p('natoms'), p('f_pred'), p('f_ref'),
        p('s_pred') if stress else None, p('s_ref') if stress else None, KBAR, sums.data_ptr(),
        torch.cuda.current_stream().cuda_stream))
    return sums


def oracle(c, criterion, stress=True):
    return error_sums_torch(criterion, DELTA, c['e_pred'], c['e_ref'], c['natoms'], c['f_pred'], c['f_ref'],
                            c['s_pred'] if stress else None, c['s_ref'] if stress else None, KBAR).cpu().numpy()


def close(got, want):
    print('kernel', got, '\ntorch ', want, '\nrel   ', np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[COUNTS], want[COUNTS])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))


def zeros():
    return torch.zeros(_lib.ERR_SUMS, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('criterion', [0, 1], ids=['mse', 'huber'])
@pytest.mark.parametrize('stress', [True, False], ids=['stress', 'no-stress'])
@pytest.mark.parametrize('shape', [(1, 1), (3, 257), (9, 3000)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_kernel_equals_the_torch_sums(shape, stress, criterion):
    c = case(*shape, seed=7)
    want = oracle(c, criterion, stress)
    got = kernel(c, criterion, zeros(), stress).cpu().numpy()
    close(got, want)
    if not stress:
        assert np.all(got[_lib.ERRQ_STRESS * NS:] == 0)
    if shape[1] >= 257:   # the labels that were dropped, and Huber's two branches, are in play
        o = _lib.ERRQ_FORCE * NS
        assert got[o] < 3 * shape[1] and got[o + 1] < shape[1]
        d = (c['f_pred'].double() - c['f_ref'].double()).abs()
        d = d[~torch.isnan(c['f_ref'])]
        assert bool((d < DELTA).any()) and bool((d > DELTA).any())
    # two runs from a zeroed buffer: equal bits
    again = kernel(c, criterion, zeros(), stress).cpu().numpy()
    assert np.array_equal(got, again)


def test_an_unlabelled_batch_changes_no_bit():
    c = case(9, 3000, seed=7)
    sums = kernel(c, 1, zeros())
    before = sums.cpu().numpy().copy()
    u = case(9, 3000, seed=8, all_nan=True)
    assert bool(torch.isnan(u['e_pred']).any()) and bool(torch.isinf(u['f_pred']).any())
    kernel(u, 1, sums)
    assert np.array_equal(sums.cpu().numpy(), before)
    # and on its own it is all zeros, like the definition
    assert np.array_equal(oracle(u, 1), np.zeros(_lib.ERR_SUMS))


def test_two_calls_accumulate():
    a, b = case(9, 3000, seed=1), case(3, 257, seed=2)
    both = kernel(b, 1, kernel(a, 1, zeros())).cpu().numpy()
    close(both, kernel(a, 1, zeros()).cpu().numpy() + kernel(b, 1, zeros()).cpu().numpy())
    close(both, oracle(a, 1) + oracle(b, 1))
