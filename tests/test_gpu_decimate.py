"""Quadric decimation and the level-of-detail export chain (csrc/meshdecim.hip, d3h.meshrefine.decimate, d3h.export.lod_chain) on the MI355X: the
cases of tests/decimate_cases.py, which tests/test_decimate_emul.py runs on the host emulation of the kernel sources."""
import pytest

import decimate_cases as C

pytestmark = pytest.mark.gpu



def test_quadrics(gpu):
    C.check_quadrics(gpu)


def test_icosphere(gpu):
    C.check_icosphere(gpu)


def test_cube_of_ties(gpu):
    C.check_cube_ties(gpu)


@pytest.mark.parametrize('boundary', ['slide', 'pin'])
def test_open_sphere(gpu, boundary):
    C.check_open(gpu, boundary)


@pytest.mark.parametrize('k', [64, 65, 300])
def test_sheet_window(gpu, k):
    C.check_sheet(gpu, k)


def test_pin_mask(gpu):
    C.check_pin_mask(gpu)


def test_trim_inside_a_round(gpu):
    C.check_trim(gpu)


def test_small_and_degenerate(gpu):
    C.check_small(gpu)


def test_cube_keeps_its_shape(gpu):
    C.check_cube_shape(gpu)


@pytest.mark.parametrize('target', [320, 128])
def test_quality_against_classic(gpu, target):
    C.check_quality(gpu, target)


def test_rejects(gpu):
    C.check_rejects(gpu)


def test_lod_chain(gpu, tmp_path):
    C.check_lod_chain(gpu, tmp_path)
