"""The ten host doubles of the suite, loaded into one process (each by its own module's loader, all through native_build.load_double)."""


def load_all():
    """-> {name: CDLL}"""
    import test_delimiter_host
    import test_filter_host_double
    import test_json_host
    import test_multiline_host_double
    import test_pipeline_host_double
    from helpers import apsara_double, container_log_product, desensitize_product, prom_product, timestamp_double
    return {"delimiter": test_delimiter_host._double(), "json": test_json_host._double(), "timestamp": timestamp_double.double(),
            "apsara": apsara_double.double(), "container_log": container_log_product.double(), "desensitize": desensitize_product.double(),
            "prom": prom_product.double(), "multiline": test_multiline_host_double._double(), "pipeline": test_pipeline_host_double._double(),
            "filter": test_filter_host_double._double()}
