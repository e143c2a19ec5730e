"""tests/rare_path_cases.py without a GPU: the planner gives every case the instance it is there for, the oracle's run of every case
holds each cause of a rare-branch entry but those its id says it lacks, and no cause goes uncovered — per layout kind, and in the case
of every other instance (tests/test_gpu_rollout_rare_paths.py runs the cases)."""
import pytest

import rare_path_cases as RP
import rollout_cases as RC


@pytest.mark.parametrize("case", RP.CASES, ids=lambda c: c.id)
def test_the_planner_names_the_instance_of_every_launch(case):
    table = RP.table_of(case.table)
    for n_steps, t0 in ((case.n_steps, 0), (8, 0), (16, 8), (24, 0)):
        plan = RC.plan_of(table, case.n_envs, n_steps, t0, case.horizon, tiled=case.out == "tiled", outputs=case.out != "no_outputs",
                          start=RP.start_kw(case) or None, seed=case.seed, env_offset=case.env_offset)
        assert plan.startswith(case.expect), plan


@pytest.mark.parametrize("case", RP.CASES, ids=lambda c: c.id)
def test_the_oracle_run_holds_every_cause_the_case_does_not_lack(case):
    got = RP.census(case)
    print(case.id, got)
    assert [c for c in RP.CAUSES if got[c] == 0] == list(case.lacks)
    assert got["restart"] == case.n_envs * (1 + (case.n_steps - 7) // RP.HORIZON)  # env e at step 6 - e % 6, then every 20 steps


def test_no_cause_goes_uncovered():
    for table in ("cramped_room", "rare_unequal", "rare_mixed"):
        for n in (256, 512):
            reached = {c for case in RP.CASES if case.table == table and case.n_envs == n for c in RP.CAUSES if c not in case.lacks}
            # (no cell of cramped_room has two floor neighbours)
            assert reached == set(RP.CAUSES) - ({"replay"} if table == "cramped_room" else set()), (table, n, reached)
    for case in RP.INSTANCE_CASES + RP.HANDOVER:
        assert not set(case.lacks) - ({"replay"} if case.table == "cramped_room" else set()), case.id
