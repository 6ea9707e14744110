"""MI355X-native drop-in for the packed forward path of uci-cbcl/esm-efficient.

    from esme import ESM, ESM2, ESMC, tokenize

(the names the reference exports from `esme/__init__.py:1-4`, plus the ESM-1b/1v classes).  Put `esm-efficient_amd/` on sys.path.
"""
from esme.alphabet import tokenize, tokenize_unpad          # noqa: F401
from esme.esm import ESM, ESM2, ESM1b, ESM1v, ESMC          # noqa: F401
from esme.loss import cross_entropy, nll_loss               # noqa: F401
from esme.contacts import ContactFeatureAccumulator, ContactHead, fit_contact_head      # noqa: F401
from esme.attention_maps import AttentionMapAccumulator      # noqa: F401
from esme import optim                                      # noqa: F401  (esme.optim.AdamW: fp32 master weights, one fused HIP step)
from esme import crf                                        # noqa: F401  (esme.crf.CRF: a linear-chain CRF over packed per-residue scores)
from esme import trainer                                    # noqa: F401  (esme.trainer.RegressionModel: supervised fine-tuning)

__all__ = ['ESM', 'ESM2', 'ESM1b', 'ESM1v', 'ESMC', 'ContactHead', 'ContactFeatureAccumulator', 'fit_contact_head', 'tokenize', 'tokenize_unpad', 'cross_entropy', 'nll_loss']
__version__ = '0.1.0'
