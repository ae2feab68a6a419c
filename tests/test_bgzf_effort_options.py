"""The pipelines' bgzf_effort option is validated before anything runs (no GPU needed)."""
import pytest


def test_consensus_pipeline_rejects_bad_efforts_first(tmp_path):
    from consensuscruncher_amd.pipeline import consensus_pipeline
    missing = str(tmp_path / "missing.bam")
    with pytest.raises(ValueError):
        consensus_pipeline(missing, str(tmp_path), bgzf="device", bgzf_effort=3)
    with pytest.raises(ValueError):
        consensus_pipeline(missing, str(tmp_path), bgzf="device", bgzf_effort=0)
    with pytest.raises(ValueError):
        consensus_pipeline(missing, str(tmp_path), bgzf="host", bgzf_effort=2)
    assert not any(tmp_path.iterdir()), "nothing ran"


def test_sharded_pipeline_rejects_bad_efforts_first(tmp_path):
    from consensuscruncher_amd.sharded import sharded_pipeline
    missing = str(tmp_path / "missing.bam")
    with pytest.raises(ValueError):
        sharded_pipeline(missing, str(tmp_path), "False", None, None, bgzf="device", bgzf_effort=3)
    with pytest.raises(ValueError):
        sharded_pipeline(missing, str(tmp_path), "False", None, None, bgzf="host", bgzf_effort=2)
