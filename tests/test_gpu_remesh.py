"""Collapse, flip, smoothing and reprojection (csrc/meshremesh.hip, d3h/meshrefine.py) on the MI355X: the cases of
tests/remesh_cases.py, which tests/test_remesh_emul.py runs on the host emulation of the kernel sources."""
import pytest
import torch

import remesh_cases as C

pytestmark = pytest.mark.gpu


def test_small_and_degenerate(gpu):
    C.check_small(gpu)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_strip_of_ties(gpu, dtype):
    C.check_strip(gpu, dtype)


@pytest.mark.parametrize('k', [64, 65, 300])
def test_sheet_candidates(gpu, k):
    C.check_sheet(gpu, k, torch.int32 if k == 65 else torch.int64)


def test_pin_mask(gpu):
    C.check_pin_mask(gpu)


@pytest.mark.parametrize('open_cap', [False, True])
def test_sphere_steps(gpu, open_cap):
    C.check_sphere_steps(gpu, open_cap)


def test_reproject(gpu):
    C.check_reproject(gpu)


@pytest.mark.parametrize('open_cap', [False, True])
def test_isotropic_remesh(gpu, open_cap):
    C.check_isotropic(gpu, open_cap)


def test_rejects(gpu):
    C.check_rejects(gpu)


def test_wiring(gpu, tmp_path):
    C.check_wiring(gpu, tmp_path)
