"""Canonical per-env records of airline, emergency, space station and farm (cge_records_<env>_*) on the device.  The bodies are
tests/_lane_records.py."""
import pytest

import _lane_records as lr
from _lane_kit import cge  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", lr.KINDS)
def test_streams_are_the_references(cge, kind):
    lr.streams_are_the_references(cge, kind)


@pytest.mark.parametrize("n", lr.SIZES)
@pytest.mark.parametrize("kind", lr.KINDS)
def test_records_are_canonical(cge, kind, n):
    lr.records_are_canonical(cge, kind, n)


@pytest.mark.parametrize("kind", lr.KINDS)
def test_records_move(cge, kind):
    lr.records_move(cge, kind)


@pytest.mark.parametrize("kind", lr.KINDS)
def test_refusals(cge, kind):
    lr.refusals(cge, kind)


@pytest.mark.parametrize("kind", lr.KINDS)
def test_bounds(cge, kind):
    lr.bounds(cge, kind)


@pytest.mark.parametrize("kind", lr.KINDS)
def test_existing_entry_points_are_unchanged(cge, kind):
    lr.existing_entry_points_are_unchanged(cge, kind)
