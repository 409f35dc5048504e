"""Custom environments without a GPU: the registrar keeps the source path, build_env_unit turns it into a code object
in a cache directory keyed by content, the name check refuses in-tree names, include/wd_env.h compiles alone, and the
example's host step matches three ticks worked out by hand.  hipcc cross-compiles gfx950, so no GPU is needed."""
import hashlib
import logging
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.rendezvous_helpers import EXAMPLE_DIR, ROOT, SOURCE, example_module, registrar_for
from warp_drive_amd import build as wd_build
from warp_drive_amd.managers import function_manager as fm_mod
from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

KERNELS = ["HipRendezvousReset", "HipRendezvousStep"]


@pytest.fixture(autouse=True)
def cache(tmp_path, monkeypatch):
    path = tmp_path / "env_cache"
    monkeypatch.setenv("WD_ENV_CACHE", str(path))
    return str(path)


def _env_class(name="Thing"):
    return type(name, (), {"name": name})


# ----------------------------------------------------------------------------------------------------- registrar
def test_registrar_keeps_and_returns_the_source_path():
    reg = EnvironmentRegistrar()
    cls = reg.add(env_backend="hip", cuda_env_src_path="/somewhere/thing_step.hip")(_env_class())
    assert reg.get("Thing", "hip") is cls and not reg.has_env("Thing", "cpu")
    assert reg.get_cuda_env_src_path("Thing") == "/somewhere/thing_step.hip"
    assert reg.get_cuda_env_src_path("thing") == "/somewhere/thing_step.hip"
    assert reg.get_cuda_env_src_path("Other") is None


def test_registrar_takes_a_list_of_backends():
    reg = EnvironmentRegistrar()
    cls = reg.add(env_backend=["cpu", "pycuda"], cuda_env_src_path="/somewhere/thing_step.cu")(_env_class())
    assert reg.get("Thing", "cpu") is cls and reg.get("Thing", "hip") is cls and reg.get("Thing", "numba") is cls
    assert reg.get_cuda_env_src_path("Thing", env_backend="pycuda") == "/somewhere/thing_step.cu"


@pytest.mark.parametrize("alias", ["hip", "pycuda", "numba"])
def test_registrar_backend_aliases(alias):
    reg = EnvironmentRegistrar()
    reg.add_cuda_env_src_path("Thing", "/somewhere/thing_step.cpp", env_backend=alias)
    for other in ("hip", "pycuda", "numba"):
        assert reg.get_cuda_env_src_path("Thing", env_backend=other) == "/somewhere/thing_step.cpp"
    with pytest.raises(AssertionError):
        reg.add_cuda_env_src_path("Thing", "/somewhere/thing_step.cpp", env_backend="cpu")


@pytest.mark.parametrize("path", ["/somewhere/thing_step.py", "/somewhere/thing_step", "thing_step.hip",
                                  "kernels/thing_step.cu"])
def test_registrar_refuses_a_bad_extension_and_a_relative_path(path):
    reg = EnvironmentRegistrar()
    with pytest.raises(ValueError, match=re.escape(path)):
        reg.add_cuda_env_src_path("Thing", path)
    with pytest.raises(ValueError, match=re.escape(path)):
        reg.add(env_backend="hip", cuda_env_src_path=path)(_env_class())
    assert reg.get_cuda_env_src_path("Thing") is None


def test_registrar_reregistration_overwrites_with_a_warning(caplog):
    reg = EnvironmentRegistrar()
    reg.add_cuda_env_src_path("Thing", "/somewhere/a.hip")
    with caplog.at_level(logging.WARNING):
        reg.add_cuda_env_src_path("Thing", "/elsewhere/b.hip")
    assert reg.get_cuda_env_src_path("Thing") == "/elsewhere/b.hip"
    assert any("/somewhere/a.hip" in r.getMessage() for r in caplog.records)


def test_registrar_add_without_a_path_behaves_as_before():
    reg = EnvironmentRegistrar()
    cls = _env_class()
    assert reg.add(env_backend="cpu")(cls) is cls
    reg.add(env_backend="numba")(cls)
    assert reg.get("Thing", "cpu") is cls and reg.get("Thing", "pycuda") is cls
    assert reg.has_env("Thing", "hip") and not reg.has_env("Other", "hip")
    assert reg.get_cuda_env_src_path("Thing") is None
    with pytest.raises(Exception, match="already registered"):
        reg.add(env_backend="hip")(cls)
    with pytest.raises(KeyError):
        reg.get("Other", "cpu")
    with pytest.raises(AssertionError):
        reg.add(env_backend="tpu")
    with pytest.raises(AssertionError):
        reg.add(env_backend="cpu")(type("Nameless", (), {}))


def test_registered_source_path_tries_the_name_as_given_then_lower_cased():
    class LowerOnly:  # a registrar in the reference's style: exact, lower-cased keys
        def get_cuda_env_src_path(self, name, env_backend="pycuda"):
            return {"thing": "/somewhere/thing.cu"}.get(name)

    assert fm_mod.registered_source_path(LowerOnly(), "Thing") == "/somewhere/thing.cu"
    assert fm_mod.registered_source_path(registrar_for(), "Rendezvous") == SOURCE
    assert fm_mod.registered_source_path(None, "Thing") is None
    assert fm_mod.registered_source_path(object(), "Thing") is None
    assert fm_mod.registered_source_path(registrar_for(), None) is None
    assert fm_mod.registered_source_path(registrar_for(), "TagGridWorld") is None


# ----------------------------------------------------------------------------------------------------- the build
def _counting_run(monkeypatch):
    calls, real = [], subprocess.run

    def run(cmd, *args, **kwargs):
        calls.append(list(cmd))
        return real(cmd, *args, **kwargs)

    monkeypatch.setattr(subprocess, "run", run)
    return calls


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


def test_build_env_unit_builds_the_example_into_the_cache(cache, monkeypatch):
    manifest_before = _sha(wd_build.MANIFEST)
    in_tree_before = sorted(os.listdir(wd_build.CSRC))
    calls = _counting_run(monkeypatch)
    path = wd_build.build_env_unit("Rendezvous", SOURCE)
    assert os.path.dirname(path) == cache and os.path.isfile(path)
    assert re.fullmatch(r"Rendezvous-[0-9a-f]{16}\.hsaco", os.path.basename(path))
    assert wd_build.kernels_in(path) == KERNELS
    compiles = [c for c in calls if "-o" in c]
    assert len(compiles) == 1
    cmd = compiles[0]
    for flag in wd_build.KERNEL_FLAGS:
        assert flag in cmd
    assert f"-I{os.path.join(ROOT, 'include')}" in cmd and f"-I{EXAMPLE_DIR}" in cmd
    assert any(c.startswith("-cuid=") for c in cmd)
    # the in-tree build is untouched: same manifest bytes, nothing new next to the in-tree objects
    assert _sha(wd_build.MANIFEST) == manifest_before
    assert sorted(os.listdir(wd_build.CSRC)) == in_tree_before
    assert not [f for f in os.listdir(cache) if f.endswith(".tmp")]
    # same content: no compiler run, same path -- although the object is now OLDER than a touched source
    del calls[:]
    os.utime(path, (1, 1))
    assert wd_build.build_env_unit("Rendezvous", SOURCE) == path
    assert calls == []


def test_an_edited_source_or_included_file_gives_another_object(tmp_path):
    work = tmp_path / "copy"
    work.mkdir()
    header = work / "rendezvous_extra.h"
    header.write_text("// nothing yet\n")
    copy = work / "rendezvous_step.hip"
    copy.write_text('#include "rendezvous_extra.h"\n' + open(SOURCE).read())
    first = wd_build.build_env_unit("Rendezvous", str(copy))
    assert wd_build.kernels_in(first) == KERNELS
    assert os.path.basename(first) != os.path.basename(wd_build.env_unit_path("Rendezvous", SOURCE))
    with open(copy, "a") as f:
        f.write("// a comment\n")
    second = wd_build.env_unit_path("Rendezvous", str(copy))
    with open(header, "a") as f:
        f.write("// a comment\n")
    third = wd_build.env_unit_path("Rendezvous", str(copy))
    assert len({first, second, third}) == 3
    # ... and so does an edit of the author's header
    assert str(header) in wd_build.unit_sources(str(copy), [str(work)])
    assert os.path.join(ROOT, "include", "wd_env.h") in wd_build.unit_sources(
        SOURCE, [os.path.join(ROOT, "include")])
    assert wd_build.build_env_unit("Rendezvous", str(copy)) == third and os.path.isfile(third)


def test_a_compiler_error_raises_with_hipcc_s_message_and_leaves_nothing(tmp_path, cache):
    bad = tmp_path / "broken_step.hip"
    bad.write_text('#include "wd_env.h"\nWD_ENV_KERNEL void HipBrokenStep(int *p) { this is not a statement }\n')
    with pytest.raises(RuntimeError) as err:
        wd_build.build_env_unit("Broken", str(bad))
    text = str(err.value)
    assert str(bad) in text and "error:" in text and "broken_step.hip:2" in text
    left = [f for f in os.listdir(cache) if f.endswith(".hsaco") or ".tmp" in f]
    assert left == []


def test_a_missing_source_is_reported(tmp_path):
    with pytest.raises(FileNotFoundError, match="nowhere_step.hip"):
        wd_build.build_env_unit("Nowhere", str(tmp_path / "nowhere_step.hip"))


def test_a_kernel_with_an_in_tree_name_is_refused_at_load(tmp_path):
    """`testkernel` lives in the in-tree build (csrc/kernels/dummy_env.hip); the check reads files only"""
    owners = wd_build.in_tree_kernel_owners()
    assert "testkernel" in owners and "reset_when_done_fused" in owners
    clash = tmp_path / "clash_step.hip"
    clash.write_text('#include "wd_env.h"\nWD_ENV_KERNEL void testkernel(int *p) { p[wd_agent_id()] = 0; }\n'
                     "WD_ENV_KERNEL void HipClashStep(int *p) { p[wd_agent_id()] = 1; }\n")
    hsaco = wd_build.build_env_unit("Clash", str(clash))
    with pytest.raises(ValueError) as err:
        fm_mod.check_custom_kernel_names(hsaco, str(clash))
    assert "testkernel" in str(err.value) and str(clash) in str(err.value) and owners["testkernel"] in str(err.value)
    # the example's names are free
    fm_mod.check_custom_kernel_names(wd_build.build_env_unit("Rendezvous", SOURCE), SOURCE)


def test_compile_and_load_builds_the_env_unit_under_the_event_protocol(monkeypatch):
    """process 0 builds the in-tree objects AND the env's unit before it sets the Event; a process that waited for the
    Event compiles nothing and loads the object process 0 left; without a registered source nothing new happens
    (the device calls of the manager are stubbed: this is the host's protocol only)"""
    import threading

    log = []

    def manager(process_id):
        m = fm_mod.HIPFunctionManager.__new__(fm_mod.HIPFunctionManager)
        m._process_id, m._module, m._custom_module = process_id, None, None
        m.load_hip_from_binary_file = lambda default_functions_included=True: (
            log.append(("main", process_id)), setattr(m, "_module", object()))[0]
        m.load_custom_hip_from_binary_file = lambda hsaco, src=None: log.append(("custom", process_id, hsaco, src))
        return m

    monkeypatch.setattr(wd_build, "build_kernels", lambda *a, **k: log.append(("build_kernels",)))
    monkeypatch.setattr(wd_build, "build_kernels_locked", lambda *a, **k: log.append(("build_kernels_locked",)))
    calls = _counting_run(monkeypatch)
    event, reg = threading.Event(), registrar_for()
    manager(0).compile_and_load_hip(env_name="Rendezvous", customized_env_registrar=reg, event_messenger=event)
    target = wd_build.env_unit_path("Rendezvous", SOURCE)
    assert event.is_set() and os.path.isfile(target)
    assert log == [("build_kernels",), ("main", 0), ("custom", 0, target, SOURCE)]
    assert len([c for c in calls if "-o" in c]) == 1
    del log[:], calls[:]
    manager(1).compile_and_load_hip(env_name="Rendezvous", customized_env_registrar=reg, event_messenger=event)
    assert log == [("main", 1), ("custom", 1, target, SOURCE)] and calls == []
    # no Event: the file locks; no registrar, or a registrar without a path for the name: exactly the old call
    del log[:]
    manager(0).compile_and_load_hip(env_name="Rendezvous", customized_env_registrar=reg)
    manager(0).compile_and_load_hip(env_name="TagGridWorld", customized_env_registrar=reg)
    manager(0).compile_and_load_hip(env_name="Rendezvous")
    assert log == [("build_kernels_locked",), ("main", 0), ("custom", 0, target, SOURCE),
                   ("build_kernels_locked",), ("main", 0), ("build_kernels_locked",), ("main", 0)] and calls == []


def test_wd_env_h_compiles_alone(tmp_path):
    text = open(os.path.join(ROOT, "include", "wd_env.h")).read()
    assert set(re.findall(r"^\s*#include\s+(\S+)", text, re.M)) == {"<hip/hip_runtime.h>", "<stdint.h>"}
    one = tmp_path / "only_header.hip"
    one.write_text('#include "wd_env.h"\nWD_ENV_KERNEL void HipNothingStep() {}\n')
    assert wd_build.kernels_in(wd_build.build_env_unit("Nothing", str(one))) == ["HipNothingStep"]


def _code_object_metadata(hsaco):
    """{kernel: (private segment, VGPR spills, SGPR spills, static LDS, VGPRs)} from the code object's notes"""
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "env.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={hsaco}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"^\s{4}\.name:\s+(\S+)$", block, re.M)
        if name is None:
            continue
        field = lambda key: int(re.search(r"^\s{4}\." + key + r":\s+(\d+)$", block, re.M).group(1))  # noqa: E731
        out[name.group(1)] = (field("private_segment_fixed_size"), field("vgpr_spill_count"),
                              field("sgpr_spill_count"), field("group_segment_fixed_size"), field("vgpr_count"))
    return out


def test_example_kernels_use_no_scratch_and_spill_nothing():
    meta = _code_object_metadata(wd_build.build_env_unit("Rendezvous", SOURCE))
    assert sorted(meta) == KERNELS
    for name, (private, vgpr_spills, sgpr_spills, lds, vgprs) in meta.items():
        print(f"{name}: {vgprs} VGPRs, private {private}, spills {vgpr_spills} / {sgpr_spills}, static LDS {lds}")
        assert (private, vgpr_spills, sgpr_spills) == (0, 0, 0), name
        assert vgprs <= 64   # a block of 1024 threads: 16 wavefronts on 4 SIMDs
    assert meta["HipRendezvousStep"][3] == 4 * 16 and meta["HipRendezvousReset"][3] == 0


# ------------------------------------------------------------------------------------------- the example's host step
def test_host_step_against_three_ticks_worked_out_by_hand():
    """N = 3, L = 4, T = 5, wall penalty 1/4, spread limit 2.  Cells (0,0) (4,0) (2,3).
    tick 1: agent 0 moves -x into the wall, the others stay: cells unchanged, Sx 6, Sy 3,
            spreads |0-6|+|0-3| = 9, |12-6|+|0-3| = 9, |6-6|+|9-3| = 6
    tick 2: +x, -x, -y: cells (1,0) (3,0) (2,2), Sx 6, Sy 2, spreads 3+2, 3+2, 0+4
    tick 3: +x, -x, -y: cells (2,0) (2,0) (2,1), Sx 6, Sy 1, spreads 0+1, 0+1, 0+2: the largest is 2 -> done early"""
    f = np.float32
    env = example_module().Rendezvous(num_agents=3, grid_length=4, episode_length=5, wall_penalty=0.25, spread_limit=2)
    env.reset()
    env.set_cells([0, 4, 2], [0, 0, 3])
    ticks = [
        ([2, 0, 0], [0, 4, 2], [0, 0, 3], 6, 3, [9, 9, 6], [True, False, False], False),
        ([1, 2, 4], [1, 3, 2], [0, 0, 2], 6, 2, [5, 5, 4], [False, False, False], False),
        ([1, 2, 4], [2, 2, 2], [0, 0, 1], 6, 1, [1, 1, 2], [False, False, False], True),
    ]
    for t, (actions, xs, ys, sx, sy, spreads, hits, finished) in enumerate(ticks, start=1):
        obs, rew, done, _ = env.step({a: np.int32(actions[a]) for a in range(3)})
        assert env.loc_x.tolist() == xs and env.loc_y.tolist() == ys and env.loc_x.dtype == np.int32
        for a in range(3):
            want = np.array([f(xs[a]) / f(4), f(ys[a]) / f(4), f(sx) / f(12), f(sy) / f(12), f(t) / f(5)], dtype=f)
            assert obs[a].dtype == f and obs[a].tobytes() == want.tobytes(), (t, a, obs[a], want)
            reward = -f(spreads[a]) / f(12)
            if hits[a]:
                reward = reward - f(0.25)
            assert np.asarray(rew[a]).dtype == f and f(rew[a]).tobytes() == f(reward).tobytes(), (t, a)
        assert done["__all__"] is finished and env.last_max_spread == max(spreads)
    # the wall hit of tick 1, in numbers: -9/12 - 1/4
    assert float(-f(9) / f(12) - f(0.25)) == -1.0
    # without a limit the same episode runs to the time limit; reset() restarts from the drawn cells
    env = example_module().Rendezvous(num_agents=3, grid_length=4, episode_length=3, seed=5)
    first = env.reset()
    outcomes = [env.step({a: 0 for a in range(3)})[2]["__all__"] for _ in range(3)]
    assert outcomes == [False, False, True]
    again = env.reset()
    assert all(np.array_equal(first[a], again[a]) for a in range(3)) and env.timestep == 0
    assert 0 <= env.starting_x.min() and env.starting_x.max() <= 4


def test_the_example_is_not_part_of_the_in_tree_build():
    assert not any("rendezvous" in unit.lower() for unit, _ in wd_build.UNITS.values())
    assert "HipRendezvousStep" not in wd_build.in_tree_kernel_owners()
