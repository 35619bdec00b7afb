"""Quadric decimation and the level-of-detail export chain (csrc/meshdecim.hip, d3h.meshrefine.decimate, d3h.export.lod_chain) on the host emulation of the kernel sources: the
cases of tests/decimate_cases.py, which tests/test_gpu_decimate.py runs on the MI355X."""
import pytest

import decimate_cases as C



def test_quadrics(emul):
    C.check_quadrics(emul)


def test_icosphere(emul):
    C.check_icosphere(emul)


def test_cube_of_ties(emul):
    C.check_cube_ties(emul)


@pytest.mark.parametrize('boundary', ['slide', 'pin'])
def test_open_sphere(emul, boundary):
    C.check_open(emul, boundary)


@pytest.mark.parametrize('k', [64, 65, 300])
def test_sheet_window(emul, k):
    C.check_sheet(emul, k)


def test_pin_mask(emul):
    C.check_pin_mask(emul)


def test_trim_inside_a_round(emul):
    C.check_trim(emul)


def test_small_and_degenerate(emul):
    C.check_small(emul)


def test_cube_keeps_its_shape(emul):
    C.check_cube_shape(emul)


@pytest.mark.parametrize('target', [320, 128])
def test_quality_against_classic(emul, target):
    C.check_quality(emul, target)


def test_rejects(emul):
    C.check_rejects(emul)


def test_lod_chain(emul, tmp_path):
    C.check_lod_chain(emul, tmp_path)
