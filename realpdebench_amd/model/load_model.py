"""Model registry with the reference's signature (realpdebench/model/load_model.py:4):
``load_model(train_dataset, device='cpu', **kwargs)`` reads ``train_dataset[0]`` for the shapes and
switches on ``kwargs['model_name']``.  Only the MI355X-native hot-path models are registered."""
import logging

SUPPORTED = ("fno", "transolver", "galerkin_transformer", "unet", "dpot", "mwt", "deeponet", "cno", "dmd", "wdno")


def load_model(train_dataset, device="cpu", **kwargs):
    model_name = kwargs["model_name"]
    input, target = train_dataset[0]        # T, S, S, C   (load_model.py:7-9)
    input_shape = tuple(input.shape)
    output_shape = tuple(target.shape)
    logging.info(f"Loading model {model_name} with input shape {input_shape} and output shape {output_shape}")
    # opt-in of mwt, deeponet and cno to their HIP training step (``EvalByDefault.enable_training``); it never reaches a constructor
    hip_training = model_name in ("mwt", "deeponet", "cno") and kwargs.pop("hip_training", False)
    # ``sync_bn: true`` next to it (cno, deeponet): BatchNorm statistics over the global batch, so that the instance trains data-parallel
    sync_bn = model_name in ("deeponet", "cno") and kwargs.pop("sync_bn", False)
    if sync_bn and not hip_training:
        raise ValueError("sync_bn: true needs hip_training: true (it is a switch of the opt-in HIP training step)")
    if model_name == "fno":
        from .fno import FNO3d
        model = FNO3d(
            modes1=kwargs["modes1"],
            modes2=kwargs["modes2"],
            modes3=kwargs["modes3"],
            n_layers=kwargs["n_layers"],
            width=kwargs["width"],
            shape_in=input_shape,
            shape_out=output_shape,
        ).to(device)
    elif model_name == "transolver":
        from .transolver import Transolver
        model = Transolver(                                   # load_model.py:145-152
            space_dim=kwargs["space_dim"], n_layers=kwargs["n_layers"], n_hidden=kwargs["n_hidden"],
            n_head=kwargs["n_head"], H=kwargs["H"], W=kwargs["W"], D=kwargs["D"], Time_Input=False, unified_pos=False,
            fun_dim=kwargs["fun_dim"], out_dim=kwargs["out_dim"], ref=kwargs["ref"], dropout=kwargs["dropout"],
            act=kwargs["act"], mlp_ratio=kwargs["mlp_ratio"], slice_num=kwargs["slice_num"],
        ).to(device)
    elif model_name == "galerkin_transformer":
        from .galerkin_transformer import GalerkinTransformer3d
        kwargs["node_feats"] = input_shape[-1]                # load_model.py:77-91
        kwargs["n_targets"] = output_shape[-1]
        kwargs["shape_in"] = input_shape
        kwargs["shape_out"] = output_shape
        kwargs.pop("config", None)
        model = GalerkinTransformer3d(**kwargs).to(device)
    elif model_name == "unet":
        from .unet import Unet3d
        model = Unet3d(dim=input_shape[1], out_channels=output_shape[-1], dim_mults=kwargs["dim_mults"],   # load_model.py:47-58
                       channels=input_shape[-1], in_time=input_shape[0], out_time=output_shape[0]).to(device)
    elif model_name == "dpot":
        from .dpot import DPOT
        keys = ("img_size", "in_channels", "out_channels", "in_timesteps", "out_timesteps", "patch_size", "embed_dim", "depth",
                "n_blocks", "modes", "mlp_ratio", "out_layer_dim", "normalize", "act", "time_agg", "n_cls", "model_type",
                "checkpoint_path")                            # load_model.py:108-131
        model = DPOT(shape_in=input_shape, shape_out=output_shape, **{k: kwargs[k] for k in keys}).to(device)
    elif model_name == "mwt":
        from .mwt import MWT3d
        kwargs["shape_in"] = input_shape                      # load_model.py:93-107
        kwargs["shape_out"] = output_shape
        kwargs.pop("config", None)
        model = MWT3d(**kwargs).to(device)
    elif model_name == "deeponet":
        from .deeponet import DeepONet
        model = DeepONet(shape_in=input_shape, shape_out=output_shape, input_channels=input_shape[-1],       # load_model.py:132-143
                         output_channels=output_shape[-1], p=kwargs["p"], dropout_rate=kwargs["dropout_rate"], device=device).to(device)
    elif model_name == "cno":
        from .cno import CNO3d
        if output_shape[0] > input_shape[0] and output_shape[0] % input_shape[0] == 0:                       # load_model.py:60-75
            out_dim_mult = output_shape[0] // input_shape[0]
        elif output_shape[0] == input_shape[0]:
            out_dim_mult = 1
        else:
            raise ValueError(f"Output shape {output_shape[1]} is not a multiple of input shape {input_shape[1]}")
        model = CNO3d(in_dim=input_shape[-1], out_dim=output_shape[-1], out_dim_mult=out_dim_mult, in_size=input_shape[2],
                      N_layers=kwargs["N_layers"]).to(device)
    elif model_name == "dmd":
        from .dmd import DMD
        keys = ("n_modes", "n_predict", "input_feature", "N_autoregressive")                                 # load_model.py:154-156
        missing = [k for k in keys if k not in kwargs]
        if missing:
            raise ValueError(f"model_name 'dmd' needs the config keys {', '.join(keys)}: missing {', '.join(missing)}")
        model = DMD(n_modes=kwargs["n_modes"], n_predict=kwargs["n_predict"], input_feature=kwargs["input_feature"],
                    n_autoregressive=kwargs["N_autoregressive"], shape_in=input_shape, shape_out=output_shape).to(device)
    elif model_name == "wdno":
        from .unet import Unet3d
        from .wdno import WDNO, WAVELETS, coef_len
        keys = ("dim", "dim_mults", "wave_type", "pad_mode", "beta_schedule", "sampling_timesteps", "ddim_sampling_eta", "dataset_root",
                "dataset_name")                                                                                 # load_model.py:24-45
        missing = [k for k in keys if k not in kwargs]
        if missing:                     # a bare model_name builds nothing here: say what a wdno.yaml carries, and what else the registry has
            raise ValueError(f"model_name 'wdno' needs the config keys {', '.join(keys)}: missing {', '.join(missing)} "
                             f"(the registry's models: {', '.join(SUPPORTED)})")
        channels = 8 * (input_shape[-1] + output_shape[-1] * output_shape[0] // input_shape[0])                 # load_model.py:24-45
        if kwargs["wave_type"] not in WAVELETS:
            raise NotImplementedError(f"WDNO on MI355X: wave_type {kwargs['wave_type']!r} is not built (the configs use {', '.join(WAVELETS)})")
        # the denoiser sees the padded coefficient mesh: no frame replication, relative-position bias over Tp (wdno_libs/unet.py:510)
        stride = 2 ** len(kwargs["dim_mults"])
        Tp = -(-coef_len(input_shape[0], len(WAVELETS[kwargs["wave_type"]][0])) // stride) * stride
        base_model = Unet3d(dim=kwargs["dim"], dim_mults=kwargs["dim_mults"], channels=channels, in_time=Tp, out_time=Tp).to(device)
        model = WDNO(base_model, train_dataset, kwargs["dataset_root"], kwargs["dataset_name"], kwargs["wave_type"], kwargs["pad_mode"],
                     timesteps=1000, beta_schedule=kwargs["beta_schedule"], sampling_timesteps=kwargs["sampling_timesteps"],
                     ddim_sampling_eta=kwargs["ddim_sampling_eta"]).to(device)
    else:
        raise ValueError(f"Model {model_name} not supported by the MI355X backend (supported: {', '.join(SUPPORTED)})")
    if hip_training:
        model.enable_training(**({"sync_bn": True} if sync_bn else {}))
    return model
