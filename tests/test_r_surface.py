"""The R drop-in surface keeps the reference's formals: every function of SURVEY.md §8b that the
reference defines in vert-cor.R / ver-cor-subG.R / real-data-sims.R is defined in
R/dcor.R / R/dcor_subG.R / R/dcor_hrs.R with the same argument names, order and default
expressions.  The reference's formals are the committed fixture tests/golden/r_formals.json
(made by tests/golden/make_r_formals.py from the reference's R scripts), pinned by its digest; where
those scripts are at hand ($DCOR_REFERENCE_DIR, or a `reference` directory beside this repository)
the fixture is re-extracted and compared too.  R itself is absent: the R files are
parsed, and their .Call targets are executed through the stub R runtime (tests/test_r_shim.py)."""
import json
import os

import pytest

from rformals import parse_formals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDIR = os.path.join(ROOT, "distributed-correlation_amd", "R")
FIXTURE = os.path.join(ROOT, "tests", "golden", "r_formals.json")
OURS = {"vert-cor.R": "dcor.R", "ver-cor-subG.R": "dcor_subG.R", "real-data-sims.R": "dcor_hrs.R"}


def _ours(fname):
    with open(os.path.join(RDIR, fname), encoding="utf-8") as f:
        return parse_formals(f.read())


@pytest.mark.parametrize("script", sorted(OURS))
def test_drop_in_formals_match_reference(script):
    ref = json.load(open(FIXTURE, encoding="utf-8"))[script]
    ours = _ours(OURS[script])
    for name, args in ref.items():
        assert name in ours, f"{OURS[script]} lacks {name} ({script})"
        got = [list(a) for a in ours[name]]
        assert got == [list(a) for a in args], f"{name}: formals {got} != reference {args}"


# digest of the fixture as make_r_formals.py extracted it from the reference's scripts (it prints it)
FIXTURE_SHA256 = "2ab9d2bd9f6823f2b3e471944c1c5a4149dc091e2afbd07ae52305752e21067d"


def test_fixture_matches_reference_sources():
    """The committed fixture is the extraction of the reference's formals: it covers every function
    of the drop-in surface and has the digest recorded when it was extracted, so it cannot drift
    from the reference unnoticed; with the reference's scripts at hand it is re-extracted too."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_r_formals import SURFACE, digest, extract, reference_dir
    fixture = json.load(open(FIXTURE, encoding="utf-8"))
    assert {s: list(fns) for s, fns in fixture.items()} == SURFACE
    assert digest(fixture) == FIXTURE_SHA256
    ref = reference_dir()
    if ref is not None:
        fresh = json.loads(json.dumps(extract(ref)))   # tuples -> lists, as in the fixture
        assert fresh == fixture


def test_every_section_8b_name_is_covered():
    """SURVEY.md §8b's list of R signatures to keep, each defined by one of the three files."""
    names = {"lambda_n", "lambda_INT_n", "mixquant", "correlation_NI_subG", "ci_INT_subG",
             "ci_NI_signbatch", "ci_INT_signflip", "correlation_INT_signflip", "priv_standardize",
             "dp_mean", "dp_sd", "gen_bounded_factor", "gen_bernoulli", "run_sim_one",
             "standardize_dp", "lambda_from_priv", "lambda_receiver_from_noise", "gen_mix_gaussian",
             "gen_gaussian", "rLap", "standardize_age_bmi"}
    defined = set()
    for f in OURS.values():
        defined |= set(_ours(f))
    assert names <= defined, names - defined
