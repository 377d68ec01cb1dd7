"""The table of stage-4 estimators (corsair_amd/estimators.py) and what its readers make of it: the names and defaults, the
command-line choices, the harness' refusal of what it is not wired for, and the option checks of sym_pose_batch, which hold
whichever estimator is chosen."""
import numpy as np
import pytest

NAMES = ["ransac", "fgr", "ransac_fm", "sc2", "ppf"]
DEFAULTS = {
    "ransac": {},
    "fgr": dict(fgr_mu_floor=0.025, fgr_iterations=64, fgr_tuple_test=True),
    "ransac_fm": dict(fm_ransac_n=3, fm_edge_similarity=0.9, fm_mutual=True, fm_iterations=100000),
    "sc2": dict(sc2_compat_dist=None, sc2_seeds=1024, sc2_k=20),
    "ppf": dict(ppf_scene_side=0, ppf_dist_step=None, ppf_ref_step=5, ppf_n_cand=16, ppf_view_points=None),
}
WIRED = ["ransac", "fgr"]


def _choices(parser):
    return list(next(a for a in parser._actions if a.dest == "registration").choices)


def _zero_rows():
    z = np.zeros((0, 33), np.float32)
    return z, z, [0], z, z, [0], []


def test_names_order_and_defaults():
    from corsair_amd import estimators as E, registration as R

    assert [e.name for e in E.TABLE] == NAMES and list(E.NAMES) == NAMES
    for e in E.TABLE:
        got = dict(e.options)
        assert list(got) == list(DEFAULTS[e.name]), e.name                  # the keywords, in the order of the checkers
        for key, want in DEFAULTS[e.name].items():
            assert got[key] == want and type(got[key]) is type(want), (e.name, key, got[key])
    # the three that the facade spells out as keyword-only parameters say what the table says
    assert R.sym_pose_batch.__kwdefaults__ == dict(registration=NAMES[0], **DEFAULTS["fgr"])
    assert [e.name for e in E.TABLE if e.wired] == WIRED and list(E.WIRED) == WIRED
    assert [e.name for e in E.TABLE if not e.descriptors] == ["ppf"]
    assert [(e.name, e.k) for e in E.TABLE if e.k is not None] == [("ransac_fm", 1)]
    assert [e.name for e in E.TABLE if e.no_symmetry is not None] == ["ransac_fm", "ppf"]
    # the checkers stay where their callers look for them
    assert R.check_fm_options is E.check_fm_options and R.check_sc2_options is E.check_sc2_options
    assert R.check_ppf_options is E.check_ppf_options


@pytest.mark.parametrize("name", NAMES)
def test_parsers_and_the_harness_follow_the_table(name):
    from corsair_amd import harness as H, shapenet_eval as SE

    assert _choices(SE.build_parser()) == NAMES
    assert _choices(H.build_parser()) == WIRED
    SE.Config(registration=name).check_registration()
    if name in WIRED:
        H.Config(registration=name).check_icp()
    else:
        with pytest.raises(ValueError, match="Config.registration '%s' \\(.*, DESIGN \\d+\\) is not wired into the harness, the "
                                             "sharded evaluation or the cache format: use registration.sym_pose_batch or "
                                             "shapenet_eval" % name):
            H.Config(registration=name).check_icp()


def test_unknown_names_are_refused_with_the_whole_list():
    from corsair_amd import harness as H, registration as R, shapenet_eval as SE

    every = "must be 'ransac', 'fgr', 'ransac_fm', 'sc2' or 'ppf', got 'teaser'"
    with pytest.raises(ValueError) as e:
        R.sym_pose_batch(*_zero_rows(), registration="teaser")
    assert str(e.value) == "sym_pose_batch: registration " + every
    with pytest.raises(ValueError) as e:
        SE.Config(registration="teaser").check_registration()
    assert str(e.value) == "Config.registration " + every
    with pytest.raises(ValueError) as e:
        H.Config(registration="teaser").check_icp()
    assert str(e.value) == "Config.registration must be 'ransac' or 'fgr', got 'teaser'"


# an invalid option of one estimator under another: (option, value, the estimator chosen)
FOREIGN = [("fm_ransac_n", 10, "ransac"), ("fm_iterations", 0, "ppf"), ("sc2_k", 100, "ransac_fm"), ("sc2_seeds", -1, "fgr"),
           ("ppf_n_cand", 100, "sc2"), ("ppf_scene_side", 2, "ransac")]


@pytest.mark.parametrize("option,value,chosen", FOREIGN)
def test_options_of_an_estimator_not_chosen_are_checked(option, value, chosen):
    from corsair_amd import registration as R

    with pytest.raises(ValueError, match="sym_pose_batch: %s must be" % option):
        R.sym_pose_batch(*_zero_rows(), registration=chosen, use_symmetry=False, **{option: value})


def test_the_first_invalid_option_in_table_order_is_the_one_named():
    from corsair_amd import registration as R

    with pytest.raises(ValueError, match="fm_mutual"):
        R.sym_pose_batch(*_zero_rows(), use_symmetry=False, ppf_ref_step=0, sc2_k=1, fm_mutual=1)
    with pytest.raises(ValueError, match="sc2_k"):
        R.sym_pose_batch(*_zero_rows(), use_symmetry=False, ppf_ref_step=0, sc2_k=1)
    # the option checks stand before the body's own: use_symmetry=True is refused under "ppf", but not first
    with pytest.raises(ValueError, match="ppf_ref_step"):
        R.sym_pose_batch(*_zero_rows(), registration="ppf", ppf_ref_step=0)


def test_sc2_compat_dist_none_is_half_of_max_corr_however_it_arrives():
    """No device is needed to see which max_corr the default is taken from: half of a max_corr that is not positive is
    refused, with the value in the message."""
    from corsair_amd import registration as R

    for call in (lambda: R.sym_pose_batch(*_zero_rows(), 5, -3.0, use_symmetry=False),
                 lambda: R.sym_pose_batch(*_zero_rows(), max_corr=-3.0, use_symmetry=False),
                 lambda: R.sym_pose_batch(*_zero_rows(), 5, max_corr=-3.0, registration="sc2", use_symmetry=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "sym_pose_batch: sc2_compat_dist must be positive and finite, got -1.5"
    with pytest.raises(ValueError, match="sc2_compat_dist must be positive and finite, got -1.0"):     # given: not derived
        R.sym_pose_batch(*_zero_rows(), 5, 0.2, use_symmetry=False, sc2_compat_dist=-1.0)


def test_an_unknown_keyword_is_a_type_error():
    from corsair_amd import registration as R

    for kw in (dict(fm_ransac=3), dict(sc2_compat=0.1), dict(registration="sc2", ppf_n_cand=16, estimator="sc2")):
        with pytest.raises(TypeError):
            R.sym_pose_batch(*_zero_rows(), use_symmetry=False, **kw)
