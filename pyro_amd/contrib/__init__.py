"""Contributed modules in the reference's layout (pyro/contrib): ``forecast``."""
