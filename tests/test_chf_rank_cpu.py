"""The source layout of the 3-d f16 ranking scan (no GPU): one definition, in the header both of its kernels include."""


def test_chamfer_and_icp_share_one_ranking_scan():
    from tests.helpers import assert_one_chf_rank_scan

    assert_one_chf_rank_scan()
