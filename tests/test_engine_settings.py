"""csrc/engine_settings.h row by row: the one table of the engine's settings -- default, environment name, accepted range,
clamp -- and its two ways in, which differ on purpose.  From the environment (Engine::create) an unset variable leaves the
default, a set one is read with atoi, a value below the accepted range is ignored and one above it is clamped.  Through the
API setters (fhe_engine_set_*) a value out of range is refused with an error text and changes nothing.

The header is compiled on its own, with a plain host compiler, into tests/engine_settings_main.cpp, which prints every
setting; nothing is loaded into Python and no device is needed.  Three builds: plain, with -DFHESTR_TEST_HOOKS (the only one
that honours FHESTR_CLUSTER_TEST_FAULT), and plain under AddressSanitizer + UBSan, which runs every case again."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "engine_settings_main.cpp")
COMPILERS = ("/opt/rocm/lib/llvm/bin/clang++", "c++")

DEFAULTS = {
    "variant_selector": 0, "wide_fair_shift": 13, "dense_per_cu": 2, "cluster_fallback": 1, "keep_busy": 0, "overlap_width": 2,
    "ks_mfma_enabled": 1, "ks_chunks_override": 0, "cluster_mode": -1, "cluster_max_batch": 0xFFFFFFFF,
    "cluster_spin_limit": 1 << 22, "multibit_combine_max": 64, "multibit_workspace_cap": 0, "cluster_test_fault": 0,
    "xcd_auto_max": 16,
}
CLUSTER_MODE_TEXT = "cluster mode: -1 (automatic), 0 (never), 1 (always) or 2 (always, the 8-CU clusters of round 3)"
COMBINE_MAX_TEXT = "multibit_combine_max: at most 1024 (workspace grows by 16 MB per LWE at N = 2048)"

BUILDS = {"plain": [], "hooks": ["-DFHESTR_TEST_HOOKS"], "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    from shutil import which
    cxx = next((c for c in COMPILERS if os.path.exists(c) or which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler available")
    out = tmp_path_factory.mktemp("engine_settings")
    built = {}
    for name, flags in BUILDS.items():
        built[name] = str(out / name)
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", built[name], SOURCE], check=True)
    return built


def run(program, env=None, args=()):
    """(settings, messages) of one run: the environment holds no FHESTR_* variable but those of `env`."""
    full = {k: v for k, v in os.environ.items() if not k.startswith("FHESTR_")}
    full.update(env or {})
    r = subprocess.run([program, *args], env=full, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    settings = {k: int(v) for k, v in (ln.split("=") for ln in lines if "=" in ln and not ln.startswith(("accepted", "refused")))}
    assert list(settings) == list(DEFAULTS)
    return settings, [ln for ln in lines if ln.startswith(("accepted", "refused"))]


def expect(**changed):
    assert set(changed) <= set(DEFAULTS)
    return {**DEFAULTS, **changed}


# (variable, text, the settings that differ from the defaults): per variable one value below its accepted range, values
# inside it, one above its clamp where it has one, text that is no number
ENV_CASES = [
    ("FHESTR_LOG2_POINTS", "3", dict(variant_selector=3)),
    ("FHESTR_LOG2_POINTS", "18", dict(variant_selector=18)),
    ("FHESTR_LOG2_POINTS", "-1", dict(variant_selector=-1)),          # always accepted: Engine::create refuses an unknown selector
    ("FHESTR_LOG2_POINTS", "wide", dict()),
    ("FHESTR_WIDE_FAIR", "-1", dict()),
    ("FHESTR_WIDE_FAIR", "0", dict(wide_fair_shift=0)),
    ("FHESTR_WIDE_FAIR", "20", dict(wide_fair_shift=20)),
    ("FHESTR_WIDE_FAIR", "99", dict(wide_fair_shift=20)),
    ("FHESTR_WIDE_FAIR", "off", dict(wide_fair_shift=0)),
    ("FHESTR_DENSE_PER_CU", "-1", dict()),
    ("FHESTR_DENSE_PER_CU", "0", dict(dense_per_cu=0)),
    ("FHESTR_DENSE_PER_CU", "100000", dict(dense_per_cu=100000)),     # no upper limit
    ("FHESTR_CLUSTER_FALLBACK", "-1", dict()),
    ("FHESTR_CLUSTER_FALLBACK", "0", dict(cluster_fallback=0)),
    ("FHESTR_CLUSTER_FALLBACK", "5", dict(cluster_fallback=1)),
    ("FHESTR_KEEP_BUSY", "-1", dict()),
    ("FHESTR_KEEP_BUSY", "0", dict()),
    ("FHESTR_KEEP_BUSY", "1", dict(keep_busy=1)),
    ("FHESTR_KEEP_BUSY", "9", dict(keep_busy=1)),
    ("FHESTR_KEEP_BUSY", "yes", dict()),                              # atoi("yes") = 0
    ("FHESTR_OVERLAP_STREAMS", "-1", dict()),
    ("FHESTR_OVERLAP_STREAMS", "1", dict(overlap_width=2)),
    ("FHESTR_OVERLAP_STREAMS", "3", dict(overlap_width=3)),
    ("FHESTR_OVERLAP_STREAMS", "4", dict(overlap_width=4)),
    ("FHESTR_OVERLAP_STREAMS", "9", dict(overlap_width=4)),
    ("FHESTR_KS_MFMA", "-1", dict()),
    ("FHESTR_KS_MFMA", "0", dict(ks_mfma_enabled=0)),
    ("FHESTR_KS_MFMA", "2", dict(ks_mfma_enabled=1)),
    ("FHESTR_KS_CHUNKS", "-1", dict()),
    ("FHESTR_KS_CHUNKS", "6", dict(ks_chunks_override=6)),
    ("FHESTR_KS_CHUNKS", "100000", dict(ks_chunks_override=100000)),  # no upper limit here: the launch plan clamps it
    ("FHESTR_CLUSTER", "-2", dict()),
    ("FHESTR_CLUSTER", "-1", dict(cluster_mode=-1)),
    ("FHESTR_CLUSTER", "0", dict(cluster_mode=0)),
    ("FHESTR_CLUSTER", "1", dict(cluster_mode=1)),
    ("FHESTR_CLUSTER", "2", dict(cluster_mode=2)),
    ("FHESTR_CLUSTER", "7", dict(cluster_mode=2)),
    ("FHESTR_CLUSTER", "auto", dict(cluster_mode=0)),                 # atoi gives 0, which is "never"
    ("FHESTR_CLUSTER_SPIN_LIMIT", "-1", dict()),
    ("FHESTR_CLUSTER_SPIN_LIMIT", "3", dict(cluster_spin_limit=64)),
    ("FHESTR_CLUSTER_SPIN_LIMIT", "64", dict(cluster_spin_limit=64)),
    ("FHESTR_CLUSTER_SPIN_LIMIT", "100000", dict(cluster_spin_limit=100000)),
    ("FHESTR_MULTIBIT_COMBINE_MAX", "-1", dict()),
    ("FHESTR_MULTIBIT_COMBINE_MAX", "0", dict(multibit_combine_max=0)),
    ("FHESTR_MULTIBIT_COMBINE_MAX", "1024", dict(multibit_combine_max=1024)),
    ("FHESTR_MULTIBIT_COMBINE_MAX", "5000", dict(multibit_combine_max=1024)),
    ("FHESTR_MULTIBIT_WS_CAP", "-1", dict()),
    ("FHESTR_MULTIBIT_WS_CAP", "0", dict()),
    ("FHESTR_MULTIBIT_WS_CAP", "1", dict(multibit_workspace_cap=1)),
    ("FHESTR_MULTIBIT_WS_CAP", "2000000000", dict(multibit_workspace_cap=2000000000)),
    ("FHESTR_CLUSTER_TEST_FAULT", "5", dict()),                       # not a -DFHESTR_TEST_HOOKS build
]

# (environment, setter calls, their messages, the settings that differ from the defaults)
API_CASES = [
    ({}, ["cluster_mode=3,5"], ["refused cluster_mode: " + CLUSTER_MODE_TEXT], dict()),
    ({}, ["cluster_mode=-2,5"], ["refused cluster_mode: " + CLUSTER_MODE_TEXT], dict()),
    ({}, ["cluster_mode=2,40"], ["accepted cluster_mode"], dict(cluster_mode=2, cluster_max_batch=40)),
    ({}, ["cluster_mode=-1,0"], ["accepted cluster_mode"], dict(cluster_mode=-1, cluster_max_batch=0)),
    ({}, ["cluster_mode=1,8", "cluster_mode=3,99"], ["accepted cluster_mode", "refused cluster_mode: " + CLUSTER_MODE_TEXT],
     dict(cluster_mode=1, cluster_max_batch=8)),                      # a refused call leaves both words of the earlier one
    ({"FHESTR_CLUSTER": "2"}, ["cluster_mode=0,16"], ["accepted cluster_mode"], dict(cluster_mode=0, cluster_max_batch=16)),
    ({"FHESTR_CLUSTER": "2"}, ["cluster_mode=7,16"], ["refused cluster_mode: " + CLUSTER_MODE_TEXT], dict(cluster_mode=2)),
    ({}, ["combine_max=1025"], ["refused combine_max: " + COMBINE_MAX_TEXT], dict()),
    ({}, ["combine_max=1024"], ["accepted combine_max"], dict(multibit_combine_max=1024)),
    ({}, ["combine_max=0"], ["accepted combine_max"], dict(multibit_combine_max=0)),
    ({"FHESTR_MULTIBIT_COMBINE_MAX": "5"}, ["combine_max=4294967295"], ["refused combine_max: " + COMBINE_MAX_TEXT], dict(multibit_combine_max=5)),
    ({}, ["keep_busy=7"], ["accepted keep_busy"], dict(keep_busy=1)),
    ({}, ["keep_busy=-3"], ["accepted keep_busy"], dict(keep_busy=1)),
    ({"FHESTR_KEEP_BUSY": "1"}, ["keep_busy=0"], ["accepted keep_busy"], dict()),
]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_nothing_set_gives_every_default(programs, build):
    assert run(programs[build]) == (DEFAULTS, [])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name,text,changed", ENV_CASES, ids=[f"{n[7:]}={t}" for n, t, _ in ENV_CASES])
def test_environment_row(programs, build, name, text, changed):
    assert run(programs[build], {name: text}) == (expect(**changed), [])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_every_variable_at_once(programs, build):
    env = {"FHESTR_LOG2_POINTS": "17", "FHESTR_WIDE_FAIR": "11", "FHESTR_DENSE_PER_CU": "3", "FHESTR_CLUSTER_FALLBACK": "0",
           "FHESTR_KEEP_BUSY": "1", "FHESTR_OVERLAP_STREAMS": "3", "FHESTR_KS_MFMA": "0", "FHESTR_KS_CHUNKS": "4", "FHESTR_CLUSTER": "1",
           "FHESTR_CLUSTER_SPIN_LIMIT": "4096", "FHESTR_MULTIBIT_COMBINE_MAX": "8", "FHESTR_MULTIBIT_WS_CAP": "65536",
           "FHESTR_CLUSTER_TEST_FAULT": "9"}
    want = expect(variant_selector=17, wide_fair_shift=11, dense_per_cu=3, cluster_fallback=0, keep_busy=1, overlap_width=3, ks_mfma_enabled=0,
                  ks_chunks_override=4, cluster_mode=1, cluster_spin_limit=4096, multibit_combine_max=8, multibit_workspace_cap=65536)
    assert run(programs[build], env) == (want, [])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("env,args,messages,changed", API_CASES, ids=[" ".join(a) + ("|env" if e else "") for e, a, _, _ in API_CASES])
def test_api_setter(programs, build, env, args, messages, changed):
    assert run(programs[build], env, args) == (expect(**changed), messages)


@pytest.mark.parametrize("text,plain,hooks", [("-1", 0, 0), ("0", 0, 0), ("5", 0, 5), ("soon", 0, 0)])
def test_fault_injection_only_in_the_test_hooks_build(programs, text, plain, hooks):
    env = {"FHESTR_CLUSTER_TEST_FAULT": text}
    assert run(programs["plain"], env) == (expect(cluster_test_fault=plain), [])
    assert run(programs["hooks"], env) == (expect(cluster_test_fault=hooks), [])
    assert run(programs["hooks"]) == (DEFAULTS, [])
