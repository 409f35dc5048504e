"""Registry of environment classes by (name, backend), and of the device source of a custom environment
(reference warp_drive/utils/env_registrar.py:4-132).

The envs of this package live in the prebuilt code objects and register a class only.  An environment of the user's own
registers its class together with the ABSOLUTE path of its HIP source (`add(..., cuda_env_src_path=...)` or
`add_cuda_env_src_path`): the function manager compiles that file on first use (warp_drive_amd/build.py::build_env_unit)
and serves `Hip<Name>Step` / `Cuda<Name>Step` from it (docs/custom_environments.md)."""
import logging
import os

_SOURCE_SUFFIXES = (".hip", ".cu", ".cpp")


def _device_backend(env_backend):
    return "hip" if env_backend in ("pycuda", "numba") else env_backend


class EnvironmentRegistrar:
    _backends = ("cpu", "hip")

    def __init__(self):
        self._envs = {}
        self._src_paths = {}  # lower-cased env name -> absolute path of its device source

    def add(self, env_backend="cpu", cuda_env_src_path=None):
        """class decorator; `env_backend`: one backend or a list of them (the reference's spelling for a dual-mode class)"""
        backends = [_device_backend(b) for b in (env_backend if isinstance(env_backend, (list, tuple)) else [env_backend])]
        for backend in backends:
            assert backend in self._backends

        def register(cls):
            name = getattr(cls, "name", None)
            assert name, "the environment class needs a `name` attribute"
            for backend in backends:
                key = (name, backend)
                if key in self._envs:
                    raise Exception(f"{name} for backend {backend} is already registered")
                self._envs[key] = cls
                if backend == "hip" and cuda_env_src_path is not None:
                    self.add_cuda_env_src_path(name, cuda_env_src_path, backend)
            return cls

        return register

    def get(self, name, env_backend="cpu"):
        if env_backend in ("pycuda", "numba"):
            env_backend = "hip"
        return self._envs[(name, env_backend)]

    def has_env(self, name, env_backend="cpu"):
        if env_backend in ("pycuda", "numba"):
            env_backend = "hip"
        return (name, env_backend) in self._envs

    def add_cuda_env_src_path(self, name, cuda_env_src_path, env_backend="hip"):
        """the device source of environment `name`: an absolute path of a .hip / .cu / .cpp file"""
        assert _device_backend(env_backend) == "hip", f"unknown env_backend: {env_backend}"
        path = os.fspath(cuda_env_src_path)
        if not os.path.isabs(path) or not path.endswith(_SOURCE_SUFFIXES):
            raise ValueError(f"the device source of environment {name} must be an absolute path of a "
                             f"{' / '.join(_SOURCE_SUFFIXES)} file, not {path!r}")
        key = name.lower()
        if key in self._src_paths:
            logging.warning(f"EnvironmentRegistrar has already registered a source path for {name}; "
                            f"overwriting {self._src_paths[key]} with {path}")
        self._src_paths[key] = path

    def get_cuda_env_src_path(self, name, env_backend="hip"):
        """the registered source path of `name` (looked up without regard to case), or None"""
        assert _device_backend(env_backend) == "hip", f"unknown env_backend: {env_backend}"
        return self._src_paths.get(name.lower())
