"""CPU: Model.field_surface takes the refinement margin as a keyword whose default is the behaviour it had (one coarse cell)."""
import inspect


def test_pad_cells_is_a_keyword_with_the_old_margin_as_default():
    from hoisdf_amd.model import Model
    sig = inspect.signature(Model.field_surface).parameters
    assert sig["pad_cells"].default == 1 and sig["pad_cells"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(sig)[:8] == ["self", "feature_pyramid", "meta_info", "kind", "n", "coarse_n", "box", "return_values"]
    assert "pad_cells" in Model.field_surface.__doc__
