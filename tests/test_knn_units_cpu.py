"""The source layout of the feature k-NN (no GPU): which unit defines which kernel."""


def test_knn_units_define_eight_kernels_once():
    from tests.helpers import assert_eight_knn_kernels

    assert_eight_knn_kernels()
