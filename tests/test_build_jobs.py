"""__graft_entry__.job_limit: the build starts no more compiles side by side than MAX_JOBS / CMAKE_BUILD_PARALLEL_LEVEL allow."""
import os

import __graft_entry__ as E


def test_job_limit(monkeypatch):
    cores = max(1, os.cpu_count() or 2)
    monkeypatch.delenv("MAX_JOBS", raising=False)
    monkeypatch.delenv("CMAKE_BUILD_PARALLEL_LEVEL", raising=False)
    assert E.job_limit() == cores
    monkeypatch.setenv("MAX_JOBS", "3")
    assert E.job_limit() == min(cores, 3)
    monkeypatch.setenv("CMAKE_BUILD_PARALLEL_LEVEL", "2")
    assert E.job_limit() == min(cores, 2)
    monkeypatch.setenv("MAX_JOBS", "1000000")
    monkeypatch.delenv("CMAKE_BUILD_PARALLEL_LEVEL")
    assert E.job_limit() == cores
    for junk in ("", "many", "0", "-4"):
        monkeypatch.setenv("MAX_JOBS", junk)
        assert E.job_limit() == cores


def test_the_solve_objects_are_units_of_the_library():
    units = {obj: flags for obj, _, flags in E.hip_units()}
    for m in range(12):
        assert {"-DGR_TU_TAN1", "-DGR_TU_SOLVE", f"-DGR_TU_METRIC={m}"} <= set(units[f"kernelssolve1_m{m}.o"])
