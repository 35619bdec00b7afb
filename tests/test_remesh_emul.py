"""Collapse, flip, smoothing and reprojection (csrc/meshremesh.hip, d3h/meshrefine.py) on the host emulation of the kernel sources: the cases of
tests/remesh_cases.py, which tests/test_gpu_remesh.py runs on the MI355X."""
import pytest
import torch

import remesh_cases as C


def test_small_and_degenerate(emul):
    C.check_small(emul)


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_strip_of_ties(emul, dtype):
    C.check_strip(emul, dtype)


@pytest.mark.parametrize('k', [64, 65, 300])
def test_sheet_candidates(emul, k):
    C.check_sheet(emul, k, torch.int32 if k == 65 else torch.int64)


def test_pin_mask(emul):
    C.check_pin_mask(emul)


@pytest.mark.parametrize('open_cap', [False, True])
def test_sphere_steps(emul, open_cap):
    C.check_sphere_steps(emul, open_cap)


def test_reproject(emul):
    C.check_reproject(emul)


@pytest.mark.parametrize('open_cap', [False, True])
def test_isotropic_remesh(emul, open_cap):
    C.check_isotropic(emul, open_cap)


def test_rejects(emul):
    C.check_rejects(emul)


def test_wiring(emul, tmp_path):
    C.check_wiring(emul, tmp_path)
