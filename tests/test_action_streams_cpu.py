"""The action streams of the oracle-lockstep GPU tests (tests/_action_streams.py) stay byte for byte what they were: the SHA-256 of
every stream, at the sizes the tests use, against tests/golden/action_stream_sha256.json, which was recorded from the generators as
they stood inside the tests.  A changed stream changes which dynamics branches the GPU tests reach (test_oracle_branch_coverage.py)."""
import _action_streams as S
from conftest import golden


def test_streams_are_byte_identical_to_the_recorded_ones():
    want = golden("action_stream_sha256.json")
    got = {name: S.stream_sha256(it) for name, it in S.pinned_streams()}
    assert got == want, [k for k in want if got.get(k) != want[k]] + [k for k in got if k not in want]


def test_replay_table_names_known_streams_and_env_types():
    for rid, stream, env, okw, n, T, seed0, mode, skw, hash_rollout in S.REPLAYS:
        assert env in S.ENV_TYPES and mode in S.MODES and (stream is None or stream in S.STREAMS), rid
        assert stream is not None or hash_rollout is not None, rid
    assert len({r[0] for r in S.REPLAYS}) == len(S.REPLAYS)
