"""Canonical per-env records of airline, emergency, space station and farm (cge_records_<env>_*): what needs no GPU.  The bodies are
tests/_lane_records.py."""
import pytest

import _lane_records as lr


@pytest.mark.parametrize("kind", lr.KINDS)
def test_abi_is_declared_exported_and_bound(kind):
    lr.abi_is_declared_exported_and_bound(kind)


def test_record_sizes_follow_the_layout_rule():
    lr.record_sizes_follow_the_layout_rule()


def test_no_records_kernel_uses_scratch(tmp_path):
    lr.no_records_kernel_uses_scratch(tmp_path)


@pytest.mark.parametrize("kind", lr.KINDS)
def test_ready_marks_stay_within_the_export(kind):
    lr.ready_marks_stay_within_the_export(kind)


def test_parse_reads_a_hand_made_record():
    lr.parse_reads_a_hand_made_record()
