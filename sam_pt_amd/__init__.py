"""sam_pt_amd: SAM-PT on the MI355X.  Submodules are imported on demand; the one name exported here resolves lazily, so
``import sam_pt_amd`` stays as cheap as it was."""


def __getattr__(name):
    if name == "SuperGluePointTracker":
        from .point_tracker import SuperGluePointTracker
        return SuperGluePointTracker
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
